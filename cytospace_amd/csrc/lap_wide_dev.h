// lap_wide_dev.h -- what the wide solver's three translation units share (lap_wide.hip: the searches; lap_wide_rr.hip: reduction
// transfer and row reduction; lap_wide_drv.hip: the host driver): the kernels' argument block, the wave-level helpers, the LAYOUT of
// the solver's buffers (one definition for the kernels' accessors and the driver's sizes and fills), the pinned-memory pool of the
// launch functions, and the launch functions themselves.  Internal: lap_jv.hip sees lap_wide.h only.
#pragma once
#include "lap_dev.h"
#include "lap_wide.h"
#include <algorithm>
#include <atomic>
#include <chrono>
#include <mutex>
#include <thread>
#include <vector>

namespace cyto {

// One problem of a batch: the kernels' argument block.  Every pointer is device memory; the work arrays are the driver's (SolveJob).
//   v, u, cassign   [n] prices, row duals (written at the end), c[colsol[j]][j] per column
//   label           [n] 64-bit search labels (ordered distance << 32 | tight-hop count << 20 | predecessor row); all-ones between searches
//   bid             [n] 64-bit bids of a row-reduction round (ordered price << 32 | row); all-ones between rounds
//   rowsol, colsol  [n] (-1 = free / unassigned), matches [n] columns claimed per row by the column reduction
//   act0, act1      [n] active-row lists of the row-reduction rounds;  freerows [n];  touched [n] columns labelled in a search
//   slot_j, slot_p, slot_c  [n] per active slot: the bid's column (-1 = retired), price, raw cost of that entry
//   cache_col/val   [n][64] row caches (lap_jv.hip: build_caches)
//   cache_red       [n][64] the embedded searches' copy of the caches: fl(cache_val - v[cache_col]) per valid entry, kept current by the
//                   commits; inv_off [n + 1], inv_ent: per column, the cache entries that hold it (bits of its raw cost << 32 |
//                   row << 6 | slot), CSR.  Null where the embedded form cannot run
//   emb_longest     the longest inverse list (one word, written by embed_scan), or null.  Not null: the driver has enqueued the
//                   embedded kernel AND its plain twin, and each decides on the device whether it is the one to run (EMB_GATE)
//   misc            the status block (lap_dev.h: LapStatus)
//   same_prev       [n] 1 = the row equals the row before it (runs of identical rows: CytoSPACE repeats a spot's row per slot), or null
//   seg_sync        shared by the launch, or null: [0] workgroups that asked for fresh caches (zeroed by the driver before every launch
//                   of wide_arr / wide_aug), [1 + b] wide_arr: 1 = problem b's rounds paused; wide_aug: searches problem b still has to run
//   sc              2 KB, zeroed by the driver: the control block of the row-reduction phase machine (ScCtl)
//   scx             the phase machine's own arrays (wide_sc_ext_bytes(n), 256-byte aligned; the first wide_sc_ones_bytes(n) all-ones, the rest zero):
//                   scx_off_* below
//   par_groups, par searches of one problem that run at once on as many workgroups (0 / 1: one at a time) and their state (ParCtl)
//   aug_abort       several searches at once: 1 = a search that can no longer be committed ends early
//   arr_waste       wide_arr: full-row bids (with their cache refresh) of one launch after which the list rounds pause (aug_seg == 0)
//   aug_seg         when a launch of wide_aug returns to the driver for fresh row caches: -1 never, k > 0 after k searches, 0 when
//                   its full-row relaxations reach aug_waste or seg_quorum workgroups of the launch have asked (LapStatus::wide_done holds the
//                   number of searches done)
// (fields through an X-macro: the kernels read the block through a mirror struct whose pointers are typed as GLOBAL, so that
//  every access is a global_* instruction -- through pointers loaded from memory it would be a FLAT one, and flat accesses
//  also count on lgkmcnt: every LDS wait would wait for the outstanding global loads too)
#define WIDE_FIELDS(P, S)                                                                                                  \
    S(int, n) S(int64_t, ld) P(const float, cost) P(const int32_t, rowmap) P(float, v) P(float, u) P(float, cassign)          \
    P(unsigned long long, label) P(unsigned long long, bid) P(int32_t, rowsol) P(int32_t, colsol) P(int32_t, matches)          \
    P(int32_t, freerows) P(int32_t, act0) P(int32_t, act1) P(int32_t, touched) P(int32_t, slot_j) P(float, slot_p)            \
    P(float, slot_c) P(uint32_t, cache_col) P(float, cache_val) P(char, misc) S(long long, max_rounds)                     \
    P(const int32_t, same_prev) P(int32_t, seg_sync) S(int, aug_seg) S(int, aug_waste) S(int, arr_waste) S(int, seg_quorum)   \
    P(char, sc) S(int, par_groups) P(char, par) P(char, scx) P(float, cache_red) P(const int32_t, inv_off) P(const unsigned long long, inv_ent)    \
    P(const int32_t, emb_longest) S(int, aug_abort)
#define WIDE_F_PTR(T, name) T *name;
#define WIDE_F_VAL(T, name) T name;
struct WideArgs { WIDE_FIELDS(WIDE_F_PTR, WIDE_F_VAL) };

constexpr size_t WIDE_SC_BYTES = 2048;

namespace {

constexpr int WT = 1024;          // threads of the persistent workgroups: 16 waves
constexpr int WNW = WT / 64;
constexpr int RTB = 256;          // threads of the reduction-transfer workgroups

template <typename T> __device__ __forceinline__ T ld_sc1(const T *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <typename T> __device__ __forceinline__ void st_sc1(T *p, T x) { __hip_atomic_store(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int64_t wrow_off(const int32_t *__restrict__ rowmap, int i, int64_t ld) {
    return (int64_t)(rowmap ? rowmap[i] : i) * ld;
}
#define WIDE_F_GPTR(T, name) __attribute__((address_space(1))) T *name;
#define WIDE_F_COPY_PTR(T, name) a.name = (T *)g.name;
#define WIDE_F_COPY_VAL(T, name) a.name = g.name;
struct WideArgsG { WIDE_FIELDS(WIDE_F_GPTR, WIDE_F_VAL) };
static_assert(sizeof(WideArgs) == sizeof(WideArgsG), "mirror layout");
__device__ __forceinline__ WideArgs load_wide_args(const WideArgs *__restrict__ batch, int b) {
    const WideArgsG g = reinterpret_cast<const WideArgsG *>(batch)[b];
    WideArgs a;
    WIDE_FIELDS(WIDE_F_COPY_PTR, WIDE_F_COPY_VAL)
    return a;
}
__device__ __forceinline__ uint64_t lanemask_lt() { return (1ull << (threadIdx.x & 63)) - 1ull; }
// a value every lane holds alike, moved to an SGPR: what depends on it becomes scalar code (scalar branches instead of
// exec-mask regions, scalar address arithmetic) -- the compiler cannot see that e.g. the wave index is uniform
__device__ __forceinline__ int uni(int x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ uint32_t uni(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
__device__ __forceinline__ float uni(float x) { return __uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane((int)__float_as_uint(x))); }
__device__ __forceinline__ unsigned long long uni(unsigned long long x) {
    return ((unsigned long long)uni((uint32_t)(x >> 32)) << 32) | uni((uint32_t)x);
}
// One full cost row by one wave: 16 bytes per lane and step, four steps' loads in flight (rows are 16-byte aligned and their
// pitch is a multiple of four elements: lap_jv.hip stages anything else).  f(column, cost) for every column < n.
template <typename F> __device__ __forceinline__ void wave_row_sweep(const float *__restrict__ row, int n, int lane, F &&f) {
    constexpr int U = 8;                                   // 8 KB of the row in flight per wave (12 measured slower: registers): a lone load per step is latency-bound
    const int nq = (n + 3) >> 2;
    const float4 *__restrict__ r4 = reinterpret_cast<const float4 *>(row);
    for (int q0 = lane; q0 < nq; q0 += 64 * U) {
        float4 x[U];
#pragma unroll
        for (int u = 0; u < U; u++) { const int q = q0 + 64 * u; x[u] = q < nq ? r4[q] : make_float4(0.0f, 0.0f, 0.0f, 0.0f); }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int q = q0 + 64 * u, c = q * 4;
            if (q >= nq) continue;
            f(c, x[u].x);
            if (c + 1 < n) f(c + 1, x[u].y);
            if (c + 2 < n) f(c + 2, x[u].z);
            if (c + 3 < n) f(c + 3, x[u].w);
        }
    }
}
// value of lane l (wave-uniform l) without the LDS round trip of __shfl
__device__ __forceinline__ uint32_t rdlane(uint32_t x, int l) { return (uint32_t)__builtin_amdgcn_readlane((int)x, l); }
__device__ __forceinline__ float rdlane(float x, int l) { return __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(x), l)); }

}  // namespace

constexpr int HEADB = 256;             // threads of the machine's workgroups

// ------------------------------------------------------------------------------------------------------------------
// THE LAYOUT of the solver's buffers: every region is described once, here, as a byte offset computed from (n, G).  The kernels'
// accessors (sc_* in lap_wide_rr.hip; cl_* in lap_wide.hip) and the driver's sizes and fills (lap_wide_drv.hip) take their offsets
// from these functions; the searches' view of the par state (SearchView, below) keeps its own pointer arithmetic over the same
// per-column byte counts and is held against them.  Every region starts where the one before it ends (each offset is the one before
// it plus that region's size); the checks at the end hold every offset and total against the formulas written out in full.
// ------------------------------------------------------------------------------------------------------------------
// per-column arrays hold a whole number of 64s of columns: with 4-byte entries and up, every region starts 256-byte aligned
__host__ __device__ constexpr size_t sc_np(int n) { return ((size_t)n + 63) & ~(size_t)63; }

// ---- SolveJob::fws / iws (lap_wide.h): slots of n entries, as the wide solver uses them (the label and the bid are 64-bit: two slots) ----
enum { FWS_V = 0, FWS_U = 1, FWS_CASSIGN = 3, FWS_LABEL = 4, FWS_SLOTS = 6 };              // (slot 2: not used by the wide solver)
enum { IWS_ROWSOL = 0, IWS_COLSOL = 1, IWS_MATCHES = 2, IWS_FREEROWS = 3, IWS_ACT0 = 4, IWS_ACT1 = 5, IWS_TOUCHED = 6, IWS_SLOT_J = 7, IWS_BID = 8,
       IWS_SLOTS = 10 };

// ---- WideArgs.scx, the phase machine's own arrays: bid words [2][np] u64 | prices [2][np] u32 | bid records [2][np] ScRec (16 bytes)
// | the records' raw costs [2][np] f32.  The first wide_sc_ones_bytes(n) bytes (the bid words) start all-ones, the rest zero. ----
__host__ __device__ constexpr size_t scx_off_words(int n, int b) { return sc_np(n) * 8 * (size_t)b; }
__host__ __device__ constexpr size_t scx_off_price(int n, int k) { return sc_np(n) * (16 + 4 * (size_t)k); }
__host__ __device__ constexpr size_t scx_off_recs(int n, int b) { return sc_np(n) * (24 + 16 * (size_t)b); }
__host__ __device__ constexpr size_t scx_off_rcts(int n, int b) { return sc_np(n) * (56 + 4 * (size_t)b); }
constexpr size_t wide_sc_ones_bytes(int n) { return scx_off_words(n, 2); }
constexpr size_t wide_sc_ext_bytes(int n) { return scx_off_rcts(n, 2); }
// the one-edge searches lay their scratch over the same bytes, free once the row reduction is over (wide_claim_*, wide_aug's loop):
// claims [np] int (in 8 bytes a column) | masks [np] u64 | states [np] int2 | ClaimCtl (in 8 bytes a column) | rows left of a run [np] int
__host__ __device__ constexpr size_t scx_off_cl_claim(int) { return 0; }
__host__ __device__ constexpr size_t scx_off_cl_mask(int n) { return sc_np(n) * 8; }
__host__ __device__ constexpr size_t scx_off_cl_state(int n) { return sc_np(n) * 16; }
__host__ __device__ constexpr size_t scx_off_cl_ctl(int n) { return sc_np(n) * 24; }
__host__ __device__ constexpr size_t scx_off_cl_rem(int n) { return sc_np(n) * 32; }
constexpr size_t scx_cl_end(int n) { return scx_off_cl_rem(n) + sc_np(n) * 4; }

// ---- WideArgs.par, the state of several searches at once (G of them): the control block, then per search or per problem ----
struct ParCtl {
    unsigned int bar_arrive, bar_gen;
    int P[2], nplog[2], nolog[2];          // per batch parity: first conflicting search, entries of the two change logs
    int err, pad_;
    long long c_relax, c_hops, c_proc, c_dense, c_rounds, c_verify, c_batches, c_discarded, c_aborted;
};
constexpr size_t PAR_CTL_BYTES = 256;
static_assert(sizeof(ParCtl) <= PAR_CTL_BYTES, "control block");
// control block | labels G x [np] u64 | touched G x [np] | hops G x 2 [np] | claim words [np] | price log (col [np], val [np]) | owner log
// (col [np], owner [np]) | settled lists (col, distance) G x [np] u64 | path links by column (pred row, its column) G x [np] u64 | four
// links at a time G x 4 [np] u64
constexpr size_t PAR_B_LABEL = 8, PAR_B_TOUCHED = 4, PAR_B_HOPS = 2 * 4, PAR_B_CLAIM = 4, PAR_B_LOG = 4, PAR_B_SETTLED = 8, PAR_B_LINK = 8, PAR_B_LINK4 = 4 * 8;     // bytes per padded column
__host__ __device__ constexpr size_t par_off_labels(int, int) { return PAR_CTL_BYTES; }
__host__ __device__ constexpr size_t par_off_touched(int n, int G) { return par_off_labels(n, G) + (size_t)G * sc_np(n) * PAR_B_LABEL; }
__host__ __device__ constexpr size_t par_off_hops(int n, int G) { return par_off_touched(n, G) + (size_t)G * sc_np(n) * PAR_B_TOUCHED; }
__host__ __device__ constexpr size_t par_off_claim(int n, int G) { return par_off_hops(n, G) + (size_t)G * sc_np(n) * PAR_B_HOPS; }
__host__ __device__ constexpr size_t par_off_plog_col(int n, int G) { return par_off_claim(n, G) + sc_np(n) * PAR_B_CLAIM; }
__host__ __device__ constexpr size_t par_off_plog_val(int n, int G) { return par_off_plog_col(n, G) + sc_np(n) * PAR_B_LOG; }
__host__ __device__ constexpr size_t par_off_olog_col(int n, int G) { return par_off_plog_val(n, G) + sc_np(n) * PAR_B_LOG; }
__host__ __device__ constexpr size_t par_off_olog_own(int n, int G) { return par_off_olog_col(n, G) + sc_np(n) * PAR_B_LOG; }
__host__ __device__ constexpr size_t par_off_settled(int n, int G) { return par_off_olog_own(n, G) + sc_np(n) * PAR_B_LOG; }
__host__ __device__ constexpr size_t par_off_links(int n, int G) { return par_off_settled(n, G) + (size_t)G * sc_np(n) * PAR_B_SETTLED; }
__host__ __device__ constexpr size_t par_off_links4(int n, int G) { return par_off_links(n, G) + (size_t)G * sc_np(n) * PAR_B_LINK; }
constexpr size_t wide_par_state_bytes(int n, int G) { return par_off_links4(n, G) + (size_t)G * sc_np(n) * PAR_B_LINK4; }

// where a search's own arrays are: the problem's (one search at a time) or workgroup g's part of the state above (PAR)
// (the kernels' definition of the same layout, in the pointer arithmetic they have always used: taking these pointers from the par_off_*
//  functions changes the code generated for every several-searches-at-once kernel.  par_view_ok holds the two against each other, on
//  the host, for every solve that uses the state)
struct SearchView {
    unsigned long long *lbl, *setl, *link, *link4;
    int32_t *tch, *hop_i, *hop_j, *plog_col, *olog_col, *olog_own;
    uint32_t *claim;
    float *plog_val;
    __host__ __device__ __forceinline__ SearchView(const WideArgs &a, bool par, int g) {
        const int G = par ? a.par_groups : 1;
        const size_t np_ = sc_np(a.n);
        lbl = par ? reinterpret_cast<unsigned long long *>(a.par + PAR_CTL_BYTES) + (size_t)g * np_ : a.label;
        tch = par ? reinterpret_cast<int32_t *>(a.par + PAR_CTL_BYTES + (size_t)G * np_ * PAR_B_LABEL) + (size_t)g * np_ : a.touched;
        hop_i = par ? reinterpret_cast<int32_t *>(a.par + PAR_CTL_BYTES + (size_t)G * np_ * (PAR_B_LABEL + PAR_B_TOUCHED)) + (size_t)g * 2 * np_ : a.act0;
        hop_j = par ? hop_i + np_ : a.act1;
        claim = reinterpret_cast<uint32_t *>(a.par + PAR_CTL_BYTES + (size_t)G * np_ * (PAR_B_LABEL + PAR_B_TOUCHED + PAR_B_HOPS));
        plog_col = reinterpret_cast<int32_t *>(claim + np_);
        plog_val = reinterpret_cast<float *>(plog_col + np_);
        olog_col = reinterpret_cast<int32_t *>(plog_val + np_);
        olog_own = olog_col + np_;
        setl = reinterpret_cast<unsigned long long *>(olog_own + np_) + (size_t)g * np_;
        link = reinterpret_cast<unsigned long long *>(olog_own + np_) + ((size_t)G + (size_t)g) * np_;
        link4 = reinterpret_cast<unsigned long long *>(olog_own + np_) + (2 * (size_t)G + 4 * (size_t)g) * np_;
    }
};
// (a.par and a.par_groups > 1 set) the first search's view starts every region where par_off_* says, and the view one past the last
// search ends the state
inline bool par_view_ok(const WideArgs &a) {
    const int n = a.n, G = a.par_groups;
    const SearchView s0(a, true, 0), sG(a, true, G);
    auto at = [&](const void *p, size_t off) { return static_cast<const char *>(p) == a.par + off; };
    return at(s0.lbl, par_off_labels(n, G)) && at(sG.lbl, par_off_touched(n, G)) && at(s0.tch, par_off_touched(n, G)) && at(sG.tch, par_off_hops(n, G)) &&
           at(s0.hop_i, par_off_hops(n, G)) && at(sG.hop_i, par_off_claim(n, G)) && at(s0.claim, par_off_claim(n, G)) &&
           at(s0.plog_col, par_off_plog_col(n, G)) && at(s0.plog_val, par_off_plog_val(n, G)) && at(s0.olog_col, par_off_olog_col(n, G)) &&
           at(s0.olog_own, par_off_olog_own(n, G)) && at(s0.setl, par_off_settled(n, G)) && at(sG.setl, par_off_links(n, G)) &&
           at(s0.link, par_off_links(n, G)) && at(sG.link, par_off_links4(n, G)) && at(s0.link4, par_off_links4(n, G)) &&
           at(sG.link4, wide_par_state_bytes(n, G));
}

// ---- WideArgs.cache_red, the embedded form's arrays, built by the whole chip between the last cache build and the searches:
// cache_red [n][KC] | inv_off [n + 1] | counts [n + 1] (the last word: the longest list) | block sums [2 x blocks] | rank [n][KC] | inv_ent [n * KCU]
constexpr int EMB_SB = 256;             // columns per workgroup of the scan
constexpr size_t emb_a256(size_t b) { return (b + 255) / 256 * 256; }
constexpr int emb_blocks(int n) { return (n + EMB_SB - 1) / EMB_SB; }
constexpr size_t emb_off_inv(int n) { return emb_a256((size_t)n * KC * 4); }
constexpr size_t emb_off_cnt(int n) { return emb_off_inv(n) + emb_a256(((size_t)n + 1) * 4); }
constexpr size_t emb_off_bsum(int n) { return emb_off_cnt(n) + emb_a256(((size_t)n + 1) * 4); }
constexpr size_t emb_off_rank(int n) { return emb_off_bsum(n) + emb_a256((size_t)emb_blocks(n) * 8); }
constexpr size_t emb_off_ent(int n) { return emb_off_rank(n) + emb_a256((size_t)n * KC * 4); }
constexpr size_t wide_embed_bytes(int n) { return emb_off_ent(n) + emb_a256((size_t)n * KCU * 8); }
inline int32_t *emb_counts(const WideArgs &wa, int n) { return reinterpret_cast<int32_t *>(reinterpret_cast<char *>(wa.cache_red) + emb_off_cnt(n)); }

// ---- the checks: every offset and total against the formulas as they stood before the layout had one definition ----
constexpr bool scx_layout_ok(int n) {
    const size_t np = ((size_t)n + 63) & ~(size_t)63;
    return scx_off_words(n, 0) == 0 && scx_off_words(n, 1) == np * 8 && scx_off_words(n, 2) == scx_off_price(n, 0) &&
           scx_off_price(n, 1) == np * 20 && scx_off_price(n, 2) == scx_off_recs(n, 0) && scx_off_recs(n, 1) == np * 40 &&
           scx_off_recs(n, 2) == scx_off_rcts(n, 0) && scx_off_rcts(n, 1) == np * 60 &&
           wide_sc_ones_bytes(n) == (((size_t)n + 63) & ~(size_t)63) * (2 * 8) && wide_sc_ext_bytes(n) == np * (2 * 8 + 2 * 4 + 2 * 16 + 2 * 4) &&
           // the overlay: a region per array, none past the machine's arrays (36 of its 64 bytes a column)
           scx_off_cl_claim(n) + np * 4 <= scx_off_cl_mask(n) && scx_off_cl_mask(n) + np * 8 == scx_off_cl_state(n) &&
           scx_off_cl_state(n) + np * 8 == scx_off_cl_ctl(n) && scx_off_cl_ctl(n) + np * 8 == scx_off_cl_rem(n) &&
           scx_cl_end(n) <= wide_sc_ext_bytes(n);
}
constexpr bool par_layout_ok(int n, int G) {
    const size_t np = ((size_t)n + 63) & ~(size_t)63, g = (size_t)G;
    const size_t claim = 256 + g * np * 20, settled = claim + np * 20;
    return par_off_labels(n, G) == 256 && par_off_touched(n, G) == 256 + g * np * 8 && par_off_hops(n, G) == 256 + g * np * 12 &&
           par_off_claim(n, G) == claim && par_off_plog_col(n, G) == claim + np * 4 && par_off_plog_val(n, G) == claim + np * 8 &&
           par_off_olog_col(n, G) == claim + np * 12 && par_off_olog_own(n, G) == claim + np * 16 && par_off_settled(n, G) == settled &&
           par_off_links(n, G) == settled + g * np * 8 && par_off_links4(n, G) == settled + 2 * g * np * 8 &&
           par_off_touched(n, G) % 256 == 0 && par_off_hops(n, G) % 256 == 0 && par_off_claim(n, G) % 256 == 0 &&
           par_off_plog_col(n, G) % 256 == 0 && par_off_settled(n, G) % 256 == 0 && par_off_links(n, G) % 256 == 0 && par_off_links4(n, G) % 256 == 0 &&
           wide_par_state_bytes(n, G) == 256 + g * np * 8 + g * np * 4 + g * np * 8 + np * 4 + np * 8 + np * 8 + g * np * 8 + g * np * 8 + g * np * 32;
}
constexpr bool emb_layout_ok(int n) {
    return emb_off_inv(n) == emb_a256((size_t)n * KC * 4) && emb_off_cnt(n) == emb_a256((size_t)n * KC * 4) + emb_a256(((size_t)n + 1) * 4) &&
           emb_off_inv(n) % 256 == 0 && emb_off_cnt(n) % 256 == 0 && emb_off_bsum(n) % 256 == 0 && emb_off_rank(n) % 256 == 0 && emb_off_ent(n) % 256 == 0;
}
constexpr bool wide_layout_ok(int n) {
    return scx_layout_ok(n) && emb_layout_ok(n) && par_layout_ok(n, 2) && par_layout_ok(n, 16) && par_layout_ok(n, WIDE_PAR_GMAX);
}
static_assert(wide_layout_ok(1) && wide_layout_ok(63) && wide_layout_ok(64) && wide_layout_ok(65) && wide_layout_ok(50000), "layout of the wide solver's buffers");
static_assert(offsetof(ParCtl, P) == 8 && offsetof(ParCtl, nplog) == 16, "the driver fills P[0..1] behind the two barrier words");

// A few ints of pinned, device-visible host memory per driver call (the machine's launches report into it).  The blocks come from
// a small process-wide pool and go back to it when the call ends: driver threads are short-lived (batch.hip spawns them per call, the
// Python side one per device and call), so a block owned by a thread would be leaked with every call.  The pool itself is never
// freed (a process that unloads the HIP runtime at exit must not call into it from a static destructor): it holds as many blocks
// as calls were ever in flight at once.
struct PinnedPool {
    struct Block { int *p; size_t cap; int dev; hipEvent_t ev; bool pending; };     // pending: launches that write into it may still be queued (ev: behind them)
    std::mutex m;
    std::vector<Block> idle;
    static PinnedPool &get() { static PinnedPool *pool = new PinnedPool(); return *pool; }
};
struct PinnedInts {
    int *p = nullptr; size_t cap = 0;
    int dev = 0; hipEvent_t ev = nullptr; hipStream_t stream = nullptr;
    PinnedInts() = default;
    PinnedInts(const PinnedInts &) = delete;
    PinnedInts &operator=(const PinnedInts &) = delete;
    ~PinnedInts() { release(); }
    // back to the pool, usable again once everything queued on `stream` so far has run (the kernels that report into the block)
    void release() {
        if (!p) return;
        const bool pending = ev && hipEventRecord(ev, stream) == hipSuccess;
        if (!pending) (void)hipStreamSynchronize(stream);
        PinnedPool &pool = PinnedPool::get();
        try { std::lock_guard<std::mutex> lk(pool.m); pool.idle.push_back({p, cap, dev, ev, pending}); }
        catch (...) { (void)hipStreamSynchronize(stream); (void)hipHostFree(p); if (ev) (void)hipEventDestroy(ev); }
        p = nullptr; cap = 0; ev = nullptr;
    }
    int ensure(size_t count, hipStream_t used_on) {
        stream = used_on;
        if (count <= cap) return CYTO_OK;
        release();
        CYTO_HIP(hipGetDevice(&dev));
        PinnedPool &pool = PinnedPool::get();
        {
            std::lock_guard<std::mutex> lk(pool.m);
            for (size_t k = 0; k < pool.idle.size(); k++) {
                PinnedPool::Block &b = pool.idle[k];
                if (b.dev != dev || b.cap < count) continue;
                if (b.pending && hipEventQuery(b.ev) != hipSuccess) { (void)hipGetLastError(); continue; }
                p = b.p; cap = b.cap; ev = b.ev;
                pool.idle[k] = pool.idle.back(); pool.idle.pop_back();
                return CYTO_OK;
            }
        }
        const size_t want = std::max<size_t>(64, count * 2);
        CYTO_HIP(hipHostMalloc(reinterpret_cast<void **>(&p), want * sizeof(int), hipHostMallocCoherent | hipHostMallocMapped | hipHostMallocPortable));
        cap = want;
        if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); ev = nullptr; }     // (no event: release() drains the stream instead)
        return CYTO_OK;
    }
};
// The driver's wait for the chip: a few hundred polls of the pinned word back to back (a launch is a few microseconds), then the
// core is yielded between polls -- a process may run one such driver per device and sub-batch, more threads than cores.
struct SpinWait {
    unsigned polls = 0;
    void reset() { polls = 0; }
    void pause() {
        // (developer knob CYTO_SPIN_POLLS: polls before the first yield; 0 = never yield)
        static const unsigned k_spin = CYTO_KNOB("CYTO_SPIN_POLLS").set ? (unsigned)std::max(0, CYTO_KNOB("CYTO_SPIN_POLLS").value) : 512u;
        if (k_spin == 0 || ++polls < k_spin) __builtin_ia32_pause();
        else std::this_thread::yield();
    }
};

// ---- the launches of the row-reduction side, lap_wide_rr.hip (d_args: the batch's nb argument blocks in device memory; all of one n) ----
// The reduction transfer and the scale of every instance (wide_rt)
int wide_launch_rt(const WideArgs *d_args, int nb, int n, hipStream_t stream);
// The phase machine on the whole chip (one launch per round, in groups; `rebuild` is called for the problems whose row caches have gone
// stale), then wide_arr -- one workgroup per problem -- for the chain rounds and the free lists.  resume: wide_arr's chain rounds paused
// for fresh row caches -- it alone picks them up.  direct: the one problem's argument block on the host, or null
int wide_launch_arr(const WideArgs *d_args, int nb, int n, hipStream_t stream, int wipe_every, bool resume, int32_t *d_sync,
                    int (*rebuild)(void *ctx, const int32_t *flags), void *ctx, const WideArgs *direct);
// ---- the launches of the searches' side, lap_wide.hip ----
// The one-edge searches of every problem, on the whole chip, before the search kernel
int wide_launch_claims(const WideArgs *d_args, int nb, int n, hipStream_t stream, int32_t *d_sync);
// the embedded form's arrays (wa.cache_red, wa.inv_off, wa.inv_ent) from the row caches and prices as they stand
int wide_build_embedded(const WideArgs &wa, int n, hipStream_t stream);
// which of the searches' arrays live in LDS (developer knob CYTO_AUG_LDS)
void wide_aug_lds_choice(int n, bool &vlds, bool &clds);
// the searches: one workgroup per problem, or par_groups > 1 searches of the one problem at once (embed: in the embedded form)
int wide_launch_aug(const WideArgs *d_args, int nb, int n, hipStream_t stream, int par_groups, bool embed);

}  // namespace cyto
