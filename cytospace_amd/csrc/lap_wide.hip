// lap_wide.hip -- the WIDE form of the Jonker-Volgenant solve for gfx950 (MI355X), hand-written HIP.
//
// Same call it replaces as lap_jv.hip:  `_, y, _ = lapjv.lapjv(cost_scaled)`
// (/root/reference/cytospace/linear_assignment_solvers/linear_assignment_solvers.py:34-40), same four phases.  The chain
// solver of lap_jv.hip follows the classic Gauss-Seidel order (one dependent row scan after the other: one wave of one
// CU busy); this file computes the order-free restatement of oracle/jv_oracle_impl.h ("WIDE MODE"), whose phases have
// width, bit for bit:
//
//   wide_rt    REDUCTION TRANSFER, Jacobi: every row that owns exactly one column takes its margin against the
//              post-column-reduction prices (snapshot), all margins are subtracted at once; and the scale of the instance -- the
//              histogram of the rows' gaps u2 - u1 -- for the eps schedule.  A wave per row, full chip.
//   wide_sc_*  AUGMENTING ROW REDUCTION as Jacobi rounds of an auction, eps-SCALED where the instance has generic costs: eight
//              eps = 0 rounds, then up to 16 phases eps_0 / 2^k (every row unassigned at a phase's start, prices kept, the phase's
//              sequential tail cut), then a final eps = 0 phase.  The phase machine: every round ONE launch over the whole chip (a wave
//              per bid of the round before: it resolves that bid and bids at once for the row that takes its place; prices and owners
//              of the columns just bid for are read from their bid words, the arrays run one round late), the state in a control
//              block per problem, so a batch's problems run through their phases independently in the same launches.  A round is a
//              pure function of the state.
//   wide_arr   the chain rounds (<= 64 active rows) of instances that did not scale -- one 16-wave workgroup per problem, the
//              rows in registers, bids meeting in LDS -- and every problem's list of free rows for the searches.
//   wide_claim_*  the searches that are ONE EDGE (CytoSPACE's repeated spot rows: a free slot takes the next free column tied at its
//              spot's minimum) on the whole chip, before the search kernel: the serial loop's assignments by deferred acceptance.
//   wide_aug   AUGMENTATION: per free row a shortest-path search whose labels are the unique fixed point of a monotone
//              system ((distance, tight-hop count) labels), so the search is run SPECULATIVELY: every round each of the 16 waves
//              settles the best unsettled columns of the column blocks it owns and relaxes their owner rows from the
//              row caches; a label that later improves is simply settled again.  Any schedule reaches the oracle's
//              Dijkstra labels.  Row caches certify the scans (floor > final distance, checked when the search has
//              converged; rows that fail are relaxed from their full cost row and the search continues).  PAR: the searches of
//              16 consecutive free rows of ONE problem at once, a workgroup each, the conflict-free prefix committed in row order.
//
// The files: lap_wide_rr.hip has wide_rt, wide_sc_* and wide_arr with their launches; this file has the searches (wide_claim_*, wide_aug,
// the embedded form's builders, their launches); lap_wide_drv.hip is the host driver, wide_solve_batch; lap_wide_dev.h is what the three
// share (the argument block, the wave helpers, the layout of the solver's buffers, the launches' declarations).
//
// Row caches: lap_jv.hip (build_caches) -- <= 63 columns per row with their raw costs, sorted by column, and a floor
// that bounds the reduced cost of every other column for as long as prices only decrease (they do: the price update of
// this mode is clamped).
#include "lap_wide_dev.h"

namespace cyto {

namespace {

// the quads [q_lo, q_hi) of a row by one wave (a slice: the whole workgroup shares a row)
template <typename F> __device__ __forceinline__ void wave_row_sweep_q(const float *__restrict__ row, int q_lo, int q_hi, int n, int lane, F &&f) {
    constexpr int U = 4;
    const float4 *__restrict__ r4 = reinterpret_cast<const float4 *>(row);
    for (int q0 = q_lo + lane; q0 < q_hi; q0 += 64 * U) {
        float4 x[U];
#pragma unroll
        for (int u = 0; u < U; u++) { const int q = q0 + 64 * u; x[u] = q < q_hi ? r4[q] : make_float4(0.0f, 0.0f, 0.0f, 0.0f); }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int q = q0 + 64 * u, c = q * 4;
            if (q >= q_hi) continue;
            f(c, x[u].x);
            if (c + 1 < n) f(c + 1, x[u].y);
            if (c + 2 < n) f(c + 2, x[u].z);
            if (c + 3 < n) f(c + 3, x[u].w);
        }
    }
}
// Search labels (oracle/jv_oracle_impl.h, WIDE MODE): a 44-bit label value LV = ordered distance (32) | tight-hop count k (12),
// then 20 bits of identity (the predecessor row in `label`, the column itself in the block minima and in the best unassigned
// column): one unsigned 64-bit compare orders (distance, k, identity) lexicographically; key >> 32 is the ordered distance.
constexpr uint32_t LKMAX = 4095u;
__device__ __forceinline__ unsigned long long lkey(unsigned long long lv, uint32_t id) { return (lv << 20) | id; }
__device__ __forceinline__ unsigned long long lv_of(unsigned long long key) { return key >> 20; }
__device__ __forceinline__ uint32_t lid_of(unsigned long long key) { return (uint32_t)key & 0xFFFFFu; }
// the label value an edge gives: raw candidate (ordered) c_raw out of a column labelled (dord, k).  A candidate that does not
// exceed the label it comes from (a tight edge; rounding can even put it below) keeps the distance and counts one more tight hop
// -- nothing is added to the distance (LKMAX hops in a row: the next representable distance).
__device__ __forceinline__ unsigned long long edge_lv(uint32_t c_raw, uint32_t dord, uint32_t k) {
    return c_raw > dord ? ((unsigned long long)c_raw << 12)
                        : (k < LKMAX ? (((unsigned long long)dord << 12) | (k + 1u)) : ((unsigned long long)(dord + 1u) << 12));
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------------
// AUGMENTATION (oracle/jv_oracle_impl.h, wide mode): shortest paths with (distance, tight-hop count) labels, run speculatively.
//
// Per column (global, L2): label = (ordered distance << 32 | tight hops << 20 | predecessor row), all-ones = unlabelled; an atomic min on it
// keeps the smallest distance and, among equal distances, the lowest row -- the oracle's pred.
// In LDS: per 64-column block the smallest (distance, column) among its DIRTY columns (labelled, assigned, not settled at
// their current label), a dirty bit and an assigned bit per column, a dense bit per row (its cache could not certify the
// search: relaxed from the full cost row), the best unassigned column so far s_T = (distance, column).
// A round: every wave takes the best dirty column of the blocks it owns (block b belongs to wave b % 16), if its distance
// is below s_T's; clears the dirty bit, reads the label, relaxes the owner row's cached columns.  Barrier.  The block
// minimum of the block a wave took from is rebuilt.  Barrier.  No wave found work: converged.
// ------------------------------------------------------------------------------------------------------------------
// (scratch of the one-edge searches: the machine's arrays a.scx, free once the row reduction is over -- wide_claim_* below, and wide_aug's loop)
struct ClaimCtl { int changed, blocked, rounds, pad_; };
static_assert(sizeof(ClaimCtl) <= scx_off_cl_rem(1) - scx_off_cl_ctl(1), "the control block of the one-edge searches in its region, at the smallest n");
__device__ __forceinline__ int *cl_claim(const WideArgs &a) { return reinterpret_cast<int *>(a.scx + scx_off_cl_claim(a.n)); }
__device__ __forceinline__ unsigned long long *cl_mask(const WideArgs &a) { return reinterpret_cast<unsigned long long *>(a.scx + scx_off_cl_mask(a.n)); }
__device__ __forceinline__ int2 *cl_state(const WideArgs &a) { return reinterpret_cast<int2 *>(a.scx + scx_off_cl_state(a.n)); }
__device__ __forceinline__ ClaimCtl *cl_ctl(const WideArgs &a) { return reinterpret_cast<ClaimCtl *>(a.scx + scx_off_cl_ctl(a.n)); }
// per free-list position: how many rows of its run of identical rows are left from it on (itself included)
__device__ __forceinline__ int *cl_rem(const WideArgs &a) { return reinterpret_cast<int *>(a.scx + scx_off_cl_rem(a.n)); }
constexpr int AP = 2;              // columns a wave settles per round (their loads are in flight together)

size_t wide_aug_lds_bytes(int n, bool vlds, bool clds) {
    const size_t nblk = ((size_t)n + 63) / 64, nw32 = ((size_t)n + 31) / 32, npad = ((size_t)n + 3) & ~(size_t)3;
    return ((nblk * 8 + 3 * nw32 * 4 + npad * ((vlds ? 4 : 0) + (clds ? 2 : 0)) + 15) / 16) * 16;
}
bool wide_aug_vlds(int n) { return n <= 65534 && wide_aug_lds_bytes(n, true, true) + 4096 <= (size_t)LDS_DYNAMIC_MAX; }
bool wide_aug_clds(int n) { return n <= 65534 && wide_aug_lds_bytes(n, false, true) + 4096 <= (size_t)LDS_DYNAMIC_MAX; }

struct AugShared {
    unsigned long long T;          // best unassigned column: (ordered distance << 32 | tight hops << 20 | column)
    int ntouch, any[3], npk[3], fail, anydense, rootdense, doroot, f, err;
    int waste, stop;               // full-row relaxations of this launch; "return to the driver for fresh caches"
    int nhop;                      // edges of the path being flipped
    int nset;                      // PAR: entries of this search's list of settled columns
    int scans;
    int ab, nab;                   // PAR: this search was aborted in its rounds (search_end reads it); searches of this workgroup aborted so far
    int st_row[64], st_col[64];    // one-edge searches: their results, stored to global memory 64 at a time
    float st_val[64];
    // full-row relaxations of a round (an owner whose cache could not certify): queued by the wave that settled the column, done by the
    // WHOLE workgroup behind the round's barrier -- a 200-KB row at n = 50 000 took its one wave ~60 us while fifteen others waited at the
    // barrier (config c3: 40 of them were 2.4 of its searches' 6.1 ms)
    // (the queue lives in st_row / st_col / st_val: the one-edge loop between two searches and the rounds of a search never overlap, and
    //  the kernel's static LDS has no room for another 640 bytes beside the dynamic region; their count: npk[] >> 16)
};
static_assert(WNW * AP <= 32, "the queue of a round's full-row relaxations: two halves of the 64-entry staging arrays");

// ---- SEVERAL SEARCHES AT ONCE (one problem, PAR): the free rows' searches are independent until they are committed, and most of
// them are shallow (a few dozen settled columns after the scaled row reduction), so G workgroups run the searches of free rows
// f, f + 1, ..., f + G - 1 from ONE state, each with its own labels, and then commit IN ROW ORDER the longest prefix whose settled
// sets (and sinks) are pairwise disjoint -- which is exactly what running them one after the other gives:
//   a committed search lowers the prices of the columns it settled below its final distance and flips owners along its path; a later
//   search that settled none of those columns, did not end at that sink and whose own sink is not among them read nothing that
//   changed in a way it can observe (a lower price of a column only RAISES the label the search would give it, and that label was
//   already at or above the search's end; unassigned columns other than the sink keep their prices) -- its labels, sink and path are
//   the ones it would have computed after the commit.  The first search of a batch that meets an earlier one's set, and every one
//   after it, is discarded and runs again in the next batch.  Nothing of the restatement changes: same searches, same order, same bits.
// Conflicts are found without a serial pass and without a pass of their own: every search claims its columns with a RETURNING atomic max
// of (batch << 8 | 255 - g), and the word that comes back tells which of two searches of the batch to flag (search_end).  The committing
// workgroups log their price and owner changes; every workgroup applies the log to its LDS copies before the next batch.  Grid barriers:
// two per batch -- behind the claims, behind the commits -- and a third in the embedded form, wide_aug<.., EMB>, behind its repair.
// (the control block ParCtl, the state's layout and a search's view of it, SearchView: lap_wide_dev.h)
constexpr int PAR_GMAX = 64;
// -DCYTO_AUG_FIN_SPLIT (a developer build, tools/fin_split.py): the end of every batch by parts, per workgroup -- thread 0's clock at
// the boundaries, with a workgroup barrier in front of every stamp (so the parts of this build are a little longer than the plain one's)
#ifdef CYTO_AUG_FIN_SPLIT
constexpr int FS_MAXB = 2048, FS_G = 16, FS_NP = 15;
enum { FS_CLAIM, FS_WAIT1, FS_CHECK, FS_WAIT2, FS_UPDATE, FS_WALK, FS_COST, FS_RESET, FS_WAIT3, FS_REPAIR, FS_NTOUCH, FS_SETTLED, FS_HOPS, FS_ARRIVE,
       FS_ABORTED };
__device__ long long g_fs[FS_MAXB][FS_G][FS_NP];
#define FS_OK (PAR && batchno - 1 < FS_MAXB && g < FS_G)
#define FS_BEGIN() { if (PAR && tid == 0) { fs_mark = wall_clock64(); if (FS_OK) g_fs[batchno - 1][g][FS_ARRIVE] = fs_mark; } }
#define FS_LAP(part) { if (PAR) { __syncthreads(); if (tid == 0) { const long long fsn_ = wall_clock64(); if (FS_OK) g_fs[batchno - 1][g][part] = fsn_ - fs_mark; fs_mark = fsn_; } } }
#define FS_SET(part, val) { if (tid == 0 && FS_OK) g_fs[batchno - 1][g][part] = (val); }
#define FS_COUNT() atomicAdd(&s.st_col[63], 1)
#else
#define FS_BEGIN()
#define FS_LAP(part)
#define FS_SET(part, val)
#define FS_COUNT()
#endif
__device__ __forceinline__ void par_barrier(ParCtl *c, int G, unsigned &gen) {
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned arrived = atomicAdd(&c->bar_arrive, 1u) + 1u;
        if (arrived == (gen + 1u) * (unsigned)G) st_sc1(&c->bar_gen, gen + 1u);
        else {
            long long spins = 0;
            while (ld_sc1(&c->bar_gen) <= gen) {
                __builtin_amdgcn_s_sleep(2);
                if (++spins > (1ll << 26)) { atomicExch(&c->err, 2); break; }      // (a lost workgroup must not hang the device)
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    gen++;
    __syncthreads();
}

// The full-row relaxations a round of wide_aug queued (nd of them, in st_row / st_col / st_val), by the whole workgroup behind
// the round's barrier: a slice of the row per wave.  A round that queued one has settled a column: the rounds go on, and what these
// relaxations label is picked up.  Their count travels in the upper half of the round's pick counter (AugShared::npk), which every wave
// reads behind the barrier anyway: a counter of its own, read before the other two, cost every round of every search a serial LDS round
// trip (10 000-cell chunk: 10.8 -> 11.7 ms of searches that never come here).
// Rows shorter than this stay with the wave that settled the column, inside the round (a 40-KB row is ~12 us of one wave; and with that
// sweep gone from the round loop the compiler's allocation made every phase of wide_aug 7-10 % slower on the instances that have no
// full-row relaxation at all -- 10 000-cell chunk 10.8 -> 11.7 ms, profiles/r06q_coop_ab.txt).  -DCYTO_COOP_MIN_N=0: a developer build
// that takes every full row through the cooperative path (tools/run/r06r.sh runs the randomised stress on it).
#ifndef CYTO_COOP_MIN_N
#define CYTO_COOP_MIN_N 16384
#endif
constexpr int COOP_MIN_N = CYTO_COOP_MIN_N;
template <bool VLDS>
__device__ __forceinline__ void coop_dense_rows(AugShared *sp, int nd, const float *__restrict__ cost, const int32_t *__restrict__ rowmap, int64_t ld,
                                             int n, int w, int lane, unsigned long long *lbl, int32_t *tch, uint32_t *dirty,
                                             unsigned long long *bmin, const uint32_t *asg, const float *s_v, const float *v) {
    AugShared &s = *sp;
    const int nq = (n + 3) >> 2, per = (nq + WNW - 1) / WNW, q_lo = w * per, q_hi = min(nq, q_lo + per);
    for (int e = 0; e < nd; e++) {
        const int oiq = uni(s.st_row[e]), pjq = uni(s.st_row[32 + e]);
        const uint32_t dord = (uint32_t)uni(s.st_col[e]), kq = (uint32_t)uni(s.st_col[32 + e]);
        const float h = uni(s.st_val[e]);
        const float *__restrict__ row = cost + wrow_off(rowmap, oiq, ld);
        // (a full row offers hundreds of candidates below the best unassigned distance when many columns are near-equal:
        //  the label is read first -- a plain L2 load -- and the atomic follows only where it would change something)
        wave_row_sweep_q(row, q_lo, q_hi, n, lane, [&](int c, float x) {
            const float vc = VLDS ? s_v[c] : ld_sc1(v + c);
            const unsigned long long lv = edge_lv(f2ord((x - vc) - h), dord, kq);
            const unsigned long long key = lkey(lv, (uint32_t)oiq);
            if (c == pjq || lv > lv_of(s.T) || !(key < ld_sc1(lbl + c))) return;
            const unsigned long long old = atomicMin(lbl + c, key);                 // (as relax_to in wide_aug)
            if (key < old) {
                if (old == ~0ull) tch[atomicAdd(&s.ntouch, 1)] = c;
                if (lv_of(old) > lv) {
                    const unsigned long long ck = lkey(lv, (uint32_t)c);
                    if ((asg[c >> 5] >> (c & 31)) & 1u) { atomicOr(&dirty[c >> 5], 1u << (c & 31)); atomicMin(&bmin[c >> 6], ck); }
                    else atomicMin(&s.T, ck);
                }
            }
        });
    }
    __syncthreads();                                                                // (the next round reads the block minima these set)
}

// EMB (the embedded form: PAR without VLDS): a round of the other forms has a third dependent global round trip between its loads and its
// offers -- the prices of the 2 x 63 cached columns, whose addresses come out of the cache rows.  The round uses a cached entry only as
// fl(cache_val - v[col]), and prices change only at a commit, for the columns the committed search settled below its end: that difference
// sits in cache_red and arrives with the cache row; behind a batch's commits the whole launch rewrites the entries of the columns the
// price log names (embed_repair, through the inverse index), and meets at a fourth grid barrier.  Same two roundings in the same
// order: same bits.  The certificate, the full-row paths and the price update read cache_val and v as before.
// The repair: the entries of every column whose lane of `m` is set (column k, new price nv in that lane), a wave per column with
// the lanes over its list.  Out of line: its registers must not weigh on the rounds.
typedef __attribute__((address_space(1))) float gf32_t;
typedef __attribute__((address_space(1))) const int32_t gci32_t;
typedef __attribute__((address_space(1))) const unsigned long long gcu64_t;
__device__ __noinline__ void embed_repair(gf32_t *cache_red, gci32_t *inv_off, gcu64_t *inv_ent, uint64_t m, int k, float nv) {
    // (one column after the other was a chain of dependent round trips per column -- list bounds, entry, its cost, store: 2.5 ms at
    //  50 000^2.  The bounds of all 64 columns are read at once, an entry carries its cost, and eight columns' lists are in flight.)
    constexpr int U = 8;
    const int lane = threadIdx.x & 63;
    m = uni((unsigned long long)m);                                       // (an argument arrives in vector registers)
    const bool mine = (m >> lane) & 1;
    const int e0 = mine ? inv_off[k] : 0, e1 = mine ? inv_off[k + 1] : 0;
    while (m) {
        int b[U], e[U]; float x[U]; unsigned long long t[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int l = m ? __ffsll((unsigned long long)m) - 1 : 0;
            b[u] = m ? __builtin_amdgcn_readlane(e0, l) : 0;
            e[u] = m ? __builtin_amdgcn_readlane(e1, l) : 0;
            x[u] = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(nv), l));
            m &= m - 1;
        }
#pragma unroll
        for (int u = 0; u < U; u++) t[u] = b[u] + lane < e[u] ? inv_ent[b[u] + lane] : 0ull;
#pragma unroll
        for (int u = 0; u < U; u++) if (b[u] + lane < e[u]) cache_red[(uint32_t)t[u]] = __uint_as_float((uint32_t)(t[u] >> 32)) - x[u];
#pragma unroll
        for (int u = 0; u < U; u++)                                       // (lists longer than a wave: rare)
            for (int p = b[u] + 64 + lane; p < e[u]; p += 64) { const unsigned long long y = inv_ent[p]; cache_red[(uint32_t)y] = __uint_as_float((uint32_t)(y >> 32)) - x[u]; }
    }
}

// THE END OF A SEARCH (wide_aug): [PAR: claims, the conflict-free prefix of the batch;] price update and path, the new owners, reset.
// Out of line like embed_repair, and for the same reason: the search rounds must keep the registers they have.  The kernel's LDS arrives
// as typed pointers (what goes through them stays LDS instructions), the argument block is read again.
// Returns hops of the flipped path | P of the batch << 32 | (this search was committed) << 48 | (it was aborted in its rounds) << 49.
//
// PAR, the claims: every column a search settled (label below its end's) and its sink get an atomic max of (batch << 8 | 255 - g), which
// keeps the LOWEST workgroup of the LATEST batch -- and RETURNS the word it replaced.  Within a batch a column's word therefore holds the
// running lowest g of its claimants: an arrival that is no new running minimum sees a smaller g and flags ITSELF; an arrival that is a new
// running minimum sees the previous one and flags THAT; so, whatever the order of arrival, every claimant of a column but its lowest is
// flagged (P = the lowest flagged search: a minimum per thread, one atomic min per wave that saw a flag) -- exactly the searches that found "one of my columns carries another key" in a pass of their own behind a
// grid barrier before.  Same P, same committed prefix, same batches, same discarded searches.  A word of an earlier batch flags nobody.
// In the same pass the settled columns go to a list (column, ordered distance), compacted by ballot with one LDS atomic per wave and four
// steps, and to the path links: by column, (the row that labelled it, that row's column) -- rowsol of a path row is changed by no other
// search committed in the batch (their settled sets and sinks are disjoint), so the link is what the walk would read.
// The commit: wave 0 walks the path -- loads only, behind the sink's hop one 8-byte link per hop, or four links per round trip where the
// search settled 32 columns or more (see there) -- while the other waves update the prices from the list (no label, no touched column
// that is not settled); behind a barrier all threads store the new owners.
// The words of a batch's parity (P, log counts): P is written by the claims, between the LAST barrier of the batch before and this
// batch's first; read behind the first; the log counts grow behind the first and are read behind the second.  Workgroup 0 resets the
// OTHER parity's words behind the first barrier: their last readers (log counts: behind the second barrier of the batch before) passed
// it, and their next writers (claims of the next batch) wait behind this batch's second.
typedef __attribute__((address_space(3))) struct AugShared lds_aug_t;
typedef __attribute__((address_space(3))) unsigned long long lds_u64_t;
#ifndef CYTO_WALK_LINKS
#define CYTO_WALK_LINKS 1          // (0: a developer build whose walk reads label and rowsol per hop, for the comparison)
#endif
#ifndef CYTO_WALK_HOP4
#define CYTO_WALK_HOP4 1           // (0: a developer build that never takes four hops per round trip)
#endif
template <bool VLDS, bool CLDS, bool PAR>
__device__ __noinline__ unsigned long long search_end(const WideArgs *__restrict__ batch, lds_aug_t *sp, lds_u64_t *smem, int g_, int fr_, int batchno_,
                                                      unsigned pgen_, int active_) {
    constexpr bool LINKS = PAR && CYTO_WALK_LINKS;
    AugShared &s = *(AugShared *)sp;
    const int g = uni(g_), fr = uni(fr_), batchno = uni(batchno_);
    unsigned pgen = uni(pgen_);
    const bool active = uni(active_) != 0;
    // (PAR, AugShared::ab: the search was ABORTED in its rounds -- a lower search of the batch is flagged, or this one is: it has no end,
    //  claims nothing, commits nothing, resets what it touched and meets the batch's barriers like any discarded search.  No error.)
    const bool aborted = PAR && active && uni(s.ab) != 0;
    const WideArgs a = load_wide_args(batch, PAR ? 0 : blockIdx.x);
    const int n = a.n, tid = threadIdx.x, lane = tid & 63, w = uni((int)(threadIdx.x >> 6));
    const int nblk = (n + 63) / 64, nw32 = (n + 31) / 32;
    const int G = PAR ? a.par_groups : 1;
    ParCtl *pc = reinterpret_cast<ParCtl *>(a.par);
    const SearchView sv(a, PAR, g);
    unsigned long long *lbl = sv.lbl, *setl = sv.setl, *link = sv.link;
    int32_t *tch = sv.tch, *hop_i = sv.hop_i, *hop_j = sv.hop_j;
    unsigned long long *bmin = (unsigned long long *)smem;
    uint32_t *dirty = reinterpret_cast<uint32_t *>(bmin + nblk);
    uint32_t *asg = dirty + nw32;
    uint32_t *dense = asg + nw32;
    float *s_v = reinterpret_cast<float *>(dense + nw32);
    uint16_t *s_cs = reinterpret_cast<uint16_t *>(s_v + (VLDS ? ((n + 3) & ~3) : 0));
    auto getv = [&](int j) -> float { return VLDS ? s_v[j] : ld_sc1(a.v + j); };
    auto is_asg = [&](int c) -> bool { return (asg[c >> 5] >> (c & 31)) & 1u; };
#ifdef CYTO_AUG_FIN_SPLIT
    long long fs_mark = 0;
#endif
    const unsigned long long Tk = active && !aborted ? uni((unsigned long long)s.T) : ~0ull;
    const uint32_t Dord = (uint32_t)(Tk >> 32);
    const float D = ord2f(Dord);
    const int sink = (int)lid_of(Tk);
    const int nt = active ? uni(s.ntouch) : 0;
    const int par = batchno & 1;
    bool commit = true;
    int Pb = G;
    FS_BEGIN()
    if (PAR) {
        const bool have = Tk != ~0ull;
        // (an aborted search saw P <= g or sent it: once more, from the thread whose release the barrier below waits for)
        if (active && !have && tid == 0) { if (!aborted) atomicExch(&pc->err, 1); atomicMin(&pc->P[par], g); }
        FS_SET(FS_ABORTED, aborted ? 1 : 0)
        const uint32_t key = ((uint32_t)batchno << 8) | (uint32_t)(255 - g);
        // P needs only the LOWEST flagged search: a thread keeps the lowest it has seen in a register, and behind the pass a wave that
        // saw one sends ONE atomic min (the minimum of minima is the minimum).  (One atomic min per shared column before: a deep search
        // that shares thousands of columns with a lower one sent as many to P's one address, 110 us for 3 892 columns,
        // profiles/r09_batch_end_ab.txt.)
        uint32_t fmin = PAR_GMAX + 1;
        auto flag = [&](uint32_t old) {                           // old: what a claim's atomic max returned
            if ((old >> 8) == (uint32_t)batchno && old != key) {
                const uint32_t go = 255u - (old & 255u);
                fmin = umin32(fmin, (uint32_t)g > go ? (uint32_t)g : go);
            }
        };
        if (have) {
            // (four touched columns, then their four labels, then the settled ones' rows and claims in flight per thread.  Eight at a
            //  time was measured: no faster, and the registers it took in here made the search rounds 3 % slower -- the compiler's
            //  allocation of the kernel follows what this function clobbers)
            constexpr int CU_ = 4;
            for (int q0 = 0; q0 < nt; q0 += CU_ * WT) {            // (the same trips in every thread: the ballots below)
                int k[CU_], pre[CU_], cnt = 0;
                unsigned long long lb[CU_];
                uint64_t m[CU_];
                bool st[CU_];
#pragma unroll
                for (int t = 0; t < CU_; t++) { const int q = q0 + t * WT + tid; k[t] = q < nt ? ld_sc1(tch + q) : -1; }
#pragma unroll
                for (int t = 0; t < CU_; t++) lb[t] = k[t] >= 0 ? ld_sc1(lbl + k[t]) : ~0ull;
#pragma unroll
                for (int t = 0; t < CU_; t++) {
                    st[t] = k[t] >= 0 && lv_of(lb[t]) < lv_of(Tk) && is_asg(k[t]);
                    m[t] = __ballot(st[t]); pre[t] = cnt; cnt += __popcll(m[t]);
                }
                if (cnt == 0) continue;
                int rs[CU_];
#pragma unroll
                for (int t = 0; t < CU_; t++) rs[t] = LINKS && st[t] ? ld_sc1(a.rowsol + (int)lid_of(lb[t])) : -1;
                uint32_t old[CU_];
#pragma unroll
                for (int t = 0; t < CU_; t++) old[t] = st[t] ? atomicMax(sv.claim + k[t], key) : 0u;
                int base = 0;
                if (lane == 0) base = atomicAdd(&s.nset, cnt);
                base = uni(base);
#pragma unroll
                for (int t = 0; t < CU_; t++)
                    if (st[t]) {
                        setl[base + pre[t] + __popcll(m[t] & lanemask_lt())] = (lb[t] >> 32 << 32) | (uint32_t)k[t];
                        if (LINKS) link[k[t]] = ((unsigned long long)(uint32_t)rs[t] << 32) | lid_of(lb[t]);
                        flag(old[t]);
                        FS_COUNT();
                    }
            }
            if (tid == 0) flag(atomicMax(sv.claim + sink, key));
        }
        // (every lane of every wave arrives here: the trips above are the same in every thread.  The wave waits until its atomic has
        //  been performed: thread 0's release in par_barrier covers wave 0's own operations only, and the workgroup barrier in front
        //  of it is compiled without a wait for the other waves' outstanding stores and atomics -- the gfx950 assembly shows
        //  s_waitcnt lgkmcnt(0); s_barrier there.  One round trip, in the waves that saw a flag, instead of one per shared column)
        const uint32_t wfmin = wave_min_u32(fmin);
        if (wfmin <= (uint32_t)PAR_GMAX && lane == 0) {
            atomicMin(&pc->P[par], (int)wfmin);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        FS_LAP(FS_CLAIM)
        par_barrier(pc, G, pgen);
        FS_LAP(FS_WAIT1)
        Pb = uni(ld_sc1(&pc->P[par]));
        Pb = Pb < G ? Pb : G;
        if (g == 0 && tid == 0) { st_sc1(&pc->P[par ^ 1], PAR_GMAX + 1); st_sc1(&pc->nplog[par ^ 1], 0); st_sc1(&pc->nolog[par ^ 1], 0); }
        commit = active && have && g < Pb;
    }
    int nhop = 0;
    if (commit) {
        // A long path is a chain of dependent round trips (0.4 us each: 340 hops in the deepest search at 50 000^2, 2 074 on the critical
        // paths of a solve's 34 batches).  Where the search settled more than a few columns, every thread first follows the links of its
        // settled columns four deep -- the chains of all columns in flight together -- and stores the four links by column; the walk then
        // takes four hops per round trip.  A link whose row is the free row ends a chain (what follows it repeats it).
        const int nset = PAR ? uni(s.nset) : 0;
        // (one column per thread and trip: the chains of four columns per thread in flight took 40 registers more in here, and the
        //  search rounds paid for them -- see the claims)
        const bool hop4 = LINKS && CYTO_WALK_HOP4 && nset >= 32;
        if (hop4) {
            const unsigned long long END = 0xFFFFFFFF00000000ull | (uint32_t)fr;
            for (int q = tid; q < nset; q += WT) {
                const int k = (int)(uint32_t)ld_sc1(setl + q);
                unsigned long long *dst = sv.link4 + 4 * (size_t)k;
                unsigned long long e[4];
                e[0] = ld_sc1(link + k);
#pragma unroll
                for (int d = 1; d < 4; d++) e[d] = (int)(uint32_t)e[d - 1] != fr ? ld_sc1(link + (uint32_t)(e[d - 1] >> 32)) : END;
#pragma unroll
                for (int d = 0; d < 4; d++) dst[d] = e[d];       // (behind the loads: a load waits for the stores issued before it)
            }
            __syncthreads();
        }
        if (w == 0) {
            // the path, from the sink back to the free row: every lane makes the same loads, lane (hop & 63) keeps the hop, 64 hops are
            // stored at a time (no store between the loads of a hop: a load returns only after the stores before it are acknowledged)
#ifdef CYTO_AUG_FIN_SPLIT
            const long long fs_w0 = wall_clock64();
#endif
            int nh = 0, mi = 0, mj = 0;
            auto rec = [&](int ri, int rj) {
                if (lane == (nh & 63)) { mi = ri; mj = rj; }
                nh++;
                if ((nh & 63) == 0 && nh <= n) { st_sc1(hop_i + nh - 64 + lane, (int32_t)mi); st_sc1(hop_j + nh - 64 + lane, (int32_t)mj); }
            };
            int j = sink;
            int i = uni((int)lid_of(ld_sc1(lbl + sink)));            // (the sink is not settled: it has no link)
            rec(i, j);
            if (i != fr) {
                j = uni(ld_sc1(a.rowsol + i));
                while (nh < n) {
                    if (hop4) {                                      // four hops per round trip
                        unsigned long long e[4];
#pragma unroll
                        for (int t = 0; t < 4; t++) e[t] = ld_sc1(sv.link4 + 4 * (size_t)j + t);
                        bool done = false;
#pragma unroll
                        for (int t = 0; t < 4; t++)
                            if (!done) {
                                const unsigned long long lk = uni(e[t]);
                                i = (int)(uint32_t)lk; rec(i, j);
                                if (i == fr) done = true; else j = (int)(uint32_t)(lk >> 32);
                            }
                        if (done) break;
                    } else if (LINKS) {
                        const unsigned long long lk = uni(ld_sc1(link + j));
                        i = (int)(uint32_t)lk; rec(i, j);
                        if (i == fr) break;
                        j = (int)(uint32_t)(lk >> 32);
                    } else {
                        i = uni((int)lid_of(ld_sc1(lbl + j))); rec(i, j);
                        if (i == fr) break;
                        j = uni(ld_sc1(a.rowsol + i));
                    }
                }
            }
            if (nh > n) nh = n;
            if (lane < (nh & 63)) { st_sc1(hop_i + (nh & ~63) + lane, (int32_t)mi); st_sc1(hop_j + (nh & ~63) + lane, (int32_t)mj); }
            if (lane == 0) s.nhop = nh;
            if (lane == 0 && i != fr) { if (PAR) atomicExch(&pc->err, 1); else s.err = 1; }      // (a path of n hops that has not reached its row: never)
#ifdef CYTO_AUG_FIN_SPLIT
            if (lane == 0 && FS_OK) g_fs[batchno - 1][g][FS_WALK] = wall_clock64() - fs_w0;
#endif
        } else {
            // the prices of the columns settled below the end's distance: v[k] += d[k] - D, clamped (prices only decrease)
            constexpr int UT = WT - 64;
            const int ne = PAR ? uni(s.nset) : nt;
            int myscans = 0;
            for (int q0 = 0; q0 < ne; q0 += 4 * UT) {
                int k[4], pre[4], cnt = 0;
                uint32_t dord[4];
                float vk[4], nv[4];
                uint64_t m[4];
                bool up[4];
                if (PAR) {
#pragma unroll
                    for (int t = 0; t < 4; t++) {
                        const int q = q0 + t * UT + tid - 64;
                        const unsigned long long e = q < ne ? ld_sc1(setl + q) : ~0ull;
                        k[t] = (int)(uint32_t)e; dord[t] = (uint32_t)(e >> 32);
                        up[t] = q < ne && dord[t] < Dord;
                    }
                } else {
#pragma unroll
                    for (int t = 0; t < 4; t++) { const int q = q0 + t * UT + tid - 64; k[t] = q < ne ? ld_sc1(tch + q) : -1; }
#pragma unroll
                    for (int t = 0; t < 4; t++) {
                        dord[t] = k[t] >= 0 ? (uint32_t)(ld_sc1(lbl + k[t]) >> 32) : 0xFFFFFFFFu;
                        up[t] = k[t] >= 0 && dord[t] < Dord && is_asg(k[t]);
                    }
                }
#pragma unroll
                for (int t = 0; t < 4; t++) vk[t] = up[t] ? getv(k[t]) : 0.0f;
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    nv[t] = (vk[t] + ord2f(dord[t])) - D;
                    myscans += up[t] ? 1 : 0;
                    up[t] = up[t] && nv[t] < vk[t];                 // (from here on: the price changes)
                    if (up[t]) { a.v[k[t]] = nv[t]; if (VLDS) s_v[k[t]] = nv[t]; }
                    if (PAR) { m[t] = __ballot(up[t]); pre[t] = cnt; cnt += __popcll(m[t]); }
                }
                if (PAR && cnt) {                                    // the price log: its slots from one atomic per wave
                    int base = 0;
                    if (lane == 0) base = atomicAdd(&pc->nplog[par], cnt);
                    base = uni(base);
#pragma unroll
                    for (int t = 0; t < 4; t++)
                        if (up[t]) { const int e = base + pre[t] + __popcll(m[t] & lanemask_lt()); sv.plog_col[e] = k[t]; sv.plog_val[e] = nv[t]; }
                }
            }
            if (myscans) atomicAdd(&s.scans, myscans);
        }
        __syncthreads();
        FS_LAP(FS_UPDATE)
        // the new owners, their costs (inside the walk every hop would wait for its cost, an HBM access) and the owner log
        nhop = uni(s.nhop);
        for (int q0 = 0; q0 < nhop; q0 += WT) {
            const int q = q0 + tid;
            const bool hv = q < nhop;
            const int i = hv ? ld_sc1(hop_i + q) : 0, j = hv ? ld_sc1(hop_j + q) : 0;
            if (hv) {
                a.colsol[j] = i; a.rowsol[i] = j;
                if (CLDS) s_cs[j] = (uint16_t)i;
                a.cassign[j] = a.cost[wrow_off(a.rowmap, i, a.ld) + j];
            }
            if (PAR) {
                const uint64_t m = __ballot(hv);
                if (m) {
                    int base = 0;
                    if (lane == 0) base = atomicAdd(&pc->nolog[par], __popcll(m));
                    base = uni(base);
                    if (hv) { const int e = base + __popcll(m & lanemask_lt()); sv.olog_col[e] = j; sv.olog_own[e] = i; }
                }
            }
        }
        if (tid == 0) atomicOr(&asg[sink >> 5], 1u << (sink & 31));
        FS_SET(FS_HOPS, nhop)
        FS_LAP(FS_COST)
    }
    for (int q0 = 0; q0 < nt; q0 += 4 * WT) {
        int k[4];
#pragma unroll
        for (int t = 0; t < 4; t++) { const int q = q0 + t * WT + tid; k[t] = q < nt ? ld_sc1(tch + q) : -1; }
#pragma unroll
        for (int t = 0; t < 4; t++)
            if (k[t] >= 0) {
                lbl[k[t]] = ~0ull;
                atomicAnd(&dirty[k[t] >> 5], ~(1u << (k[t] & 31)));
                bmin[k[t] >> 6] = ~0ull;
            }
    }
    // (keeping the dense bits across searches was measured: fewer rounds, but more full-row relaxations -- slower)
    if (s.anydense) for (int q = tid; q < nw32; q += WT) dense[q] = 0;
    __syncthreads();
    FS_SET(FS_NTOUCH, nt)
    FS_LAP(FS_RESET)
    return (unsigned long long)(uint32_t)nhop | ((unsigned long long)(uint32_t)Pb << 32) | ((unsigned long long)(commit ? 1 : 0) << 48) |
           ((unsigned long long)(aborted ? 1 : 0) << 49);
}

constexpr int EMB_GATE = 4 * KCU;       // longest inverse list the embedded form runs with (a commit rewrites a list per repriced column)
template <bool VLDS, bool CLDS, bool PAR, bool EMB = false>
__global__ __launch_bounds__(WT) void wide_aug(const WideArgs *__restrict__ batch) {
    static_assert(!EMB || (PAR && !VLDS), "the embedded form: several searches at once, prices in global memory");
    extern __shared__ __align__(16) unsigned char w_smem[];
    __shared__ AugShared s;
    // (PAR: the launch has par_groups * stride workgroups of which every stride-th takes part: stride 1 = spread over all XCDs, 8 = one XCD)
    const int pstride = PAR ? (int)(gridDim.x / (unsigned)load_wide_args(batch, 0).par_groups) : 1;
    if (PAR && (blockIdx.x % pstride)) return;
    const int g = PAR ? uni((int)(blockIdx.x / pstride)) : 0;
    const WideArgs a = load_wide_args(batch, PAR ? 0 : blockIdx.x);
    // The gate of the embedded form, on the device: a column in thousands of caches (few cell types) -- a deep search would rewrite most
    // of cache_red.  The driver has enqueued both forms behind the build of the inverse lists; the one whose turn it is not ends here,
    // before its first barrier and before it touches the status block or the control block.  (The driver read the word back and chose
    // before: the chip waited for the host, and the search kernel was enqueued onto an idle chip.)
    if (PAR && a.emb_longest && (uni(ld_sc1(a.emb_longest)) <= EMB_GATE) != EMB) return;
    const int n = a.n, tid = threadIdx.x, lane = tid & 63, w = uni((int)(threadIdx.x >> 6));
    const int nblk = (n + 63) / 64, nw32 = (n + 31) / 32;
    // the search's own arrays: the problem's (one search at a time) or this workgroup's (PAR)
    const int G = PAR ? a.par_groups : 1;
    ParCtl *pc = reinterpret_cast<ParCtl *>(a.par);
    const SearchView sv(a, PAR, g);
    unsigned long long *lbl = sv.lbl;
    int32_t *tch = sv.tch, *plog_col = sv.plog_col, *olog_col = sv.olog_col, *olog_own = sv.olog_own;
    float *plog_val = sv.plog_val;
    unsigned pgen = 0;
    unsigned long long *bmin = reinterpret_cast<unsigned long long *>(w_smem);
    uint32_t *dirty = reinterpret_cast<uint32_t *>(bmin + nblk);
    uint32_t *asg = dirty + nw32;
    uint32_t *dense = asg + nw32;
    float *s_v = reinterpret_cast<float *>(dense + nw32);
    uint16_t *s_cs = reinterpret_cast<uint16_t *>(s_v + (VLDS ? ((n + 3) & ~3) : 0));
    const int numfree = lap_status(a.misc)->numfree;
    for (int b = tid; b < nblk; b += WT) bmin[b] = ~0ull;
    for (int q = tid; q < nw32; q += WT) { dirty[q] = 0; dense[q] = 0; }
    for (int c0 = 0; c0 < nw32 * 32; c0 += WT) {                 // assigned bits, 64 columns per wave and step
        const int c = c0 + tid;
        const uint64_t m = __ballot(c < n && a.colsol[c] >= 0);
        if (lane == 0 && (c >> 5) < nw32) { asg[c >> 5] = (uint32_t)m; if ((c >> 5) + 1 < nw32) asg[(c >> 5) + 1] = (uint32_t)(m >> 32); }
    }
    if (CLDS)
        for (int j = tid; j < n; j += WT) {
            if (VLDS) s_v[j] = a.v[j];
            const int o = a.colsol[j]; s_cs[j] = o < 0 ? (uint16_t)0xFFFFu : (uint16_t)o;
        }
    // The searches may take several launches, with the row caches rebuilt by the whole chip in between (LapStatus::wide_done = searches
    // done so far).  A cache floor bounds c - v in absolute terms, as of the build; every search lowers the prices of the columns it
    // settles and raises their rows' duals with them, so after a few DEEP searches (few-cell-type chunks: a search settles most
    // columns) the floors lie below what the next search asks for and row after row falls back to its full cost row -- while
    // fresh caches certify practically everything (10 000-cell c4 chunk: 1.14 M full-row relaxations without a rebuild, 18 000
    // with one every 32 searches).  a.aug_seg: -1 never return early; k > 0 after k searches; 0: when the full-row relaxations of
    // this launch reach a.aug_waste (what a rebuild costs), or when a.seg_quorum workgroups of the launch have asked for one.
    const int f0 = PAR ? 0 : lap_status(a.misc)->wide_done;
    if (!PAR) {
        long long *wc = lap_status(a.misc)->wide;
        if (wc[WC_AUG_LAUNCHES] > 0 && f0 >= numfree) {          // finished in an earlier launch
            if (tid == 0 && a.seg_sync) a.seg_sync[1 + blockIdx.x] = 0;
            return;
        }
    }
    if (tid == 0) { s.waste = 0; s.stop = 0; }
    if (tid == 0) { s.T = ~0ull; s.ntouch = 0; s.any[0] = 0; s.any[1] = 0; s.any[2] = 0; s.npk[0] = 0; s.npk[1] = 0; s.npk[2] = 0; s.fail = 0; s.anydense = 0; s.rootdense = 0; s.doroot = 0; s.f = f0; s.err = 0; s.scans = 0; s.nset = 0; s.ab = 0; s.nab = 0; }
    __syncthreads();
    auto getv = [&](int j) -> float { return VLDS ? s_v[j] : ld_sc1(a.v + j); };
    auto getcs = [&](int j) -> int {
        if (CLDS) { const uint16_t x = s_cs[j]; return x == 0xFFFFu ? -1 : (int)x; }
        return ld_sc1(a.colsol + j);
    };
    auto is_asg = [&](int c) -> bool { return (asg[c >> 5] >> (c & 31)) & 1u; };

    long long c_relax = 0, c_hops = 0, c_rounds = 0, c_proc = 0, c_trivial = 0, c_dense = 0, c_verify = 0;   // (thread 0 / wave leaders)
    long long t_rounds = 0, t_verify = 0, t_finish = 0, t_triv = 0, t_mark = wall_clock64();

#define AUG_LAP(acc) { const long long now_ = wall_clock64(); acc += now_ - t_mark; t_mark = now_; }
#ifdef CYTO_AUG_FIN_SPLIT
    long long fs_mark = 0;
    if (tid == 0) s.st_col[63] = 0;                              // (FS_COUNT: the settled columns of the search; PAR never stages one-edge results)
    __syncthreads();
#endif

    // a relaxation in two halves: the offer (column `col` is offered the ordered distance `co` by row `row`; returns the label
    // it replaced or lost against) and what follows from it -- first touch, dirty column, best unassigned column
    auto offer = [&](int col, unsigned long long lv, int row) -> unsigned long long {
        return atomicMin(lbl + col, lkey(lv, (uint32_t)row));
    };
    auto after_offer = [&](int col, unsigned long long lv, int row, unsigned long long old) {
        const unsigned long long key = lkey(lv, (uint32_t)row);
        if (key < old) {
            if (old == ~0ull) tch[atomicAdd(&s.ntouch, 1)] = col;
            if (lv_of(old) > lv) {                              // the label value itself dropped (not only the row of a tie)
                const unsigned long long ck = lkey(lv, (uint32_t)col);
                if (is_asg(col)) { atomicOr(&dirty[col >> 5], 1u << (col & 31)); atomicMin(&bmin[col >> 6], ck); }
                else atomicMin(&s.T, ck);
            }
        }
    };
    auto relax_to = [&](int col, unsigned long long lv, int row) { after_offer(col, lv, row, offer(col, lv, row)); };
    // behind a round's barrier (every wave of the workgroup, the idle ones too): the full-row relaxations the round queued
    // (coop_dense_rows, out of line: the rounds that queued none -- nearly all -- pay one LDS read for it)

    int f = f0;
    int ph = 0;                                                  // round flag in use (three take turns: one barrier per round)
    int rb[AP];                                                  // blocks this wave took from in the last round: their minima are due
#pragma unroll
    for (int q = 0; q < AP; q++) rb[q] = -1;
    int seg_done = 0;                                            // searches (other than one-edge ones) of this launch
    int wact = 4;                                                // waves that take part in the next round of a search (4 or all 16)
    bool announced = false;
    int fbase = 0, batchno = 1, perr = 0;                        // PAR: first free row of the batch, batch number (claim keys), error seen
    long long c_batches = 0, c_discarded = 0;
    // PAR, ending a search that can no longer be committed: once per round wave 0 reads the batch's P -- the lowest flagged
    // search so far, which only falls -- and at P <= g raises AUG_ABORT in the round's pick counter, the word every wave reads behind the
    // round's barrier anyway (a word of its own there cost every round 8 %: coop_dense_rows).  No store and no atomic in a round that
    // does not abort; no barrier, no wait: the workgroup only reaches the batch's first barrier sooner.
    // (What the rounds carry for it is ONE scalar: the kernel sits at its register cap and its allocation follows everything that lives
    //  across the round loop -- "this search was aborted" travels through AugShared::ab, the count of aborted searches through ::nab.)
    constexpr int AUG_ABORT = 1 << 30;
    const int gthr = PAR && a.aug_abort ? g : -1;                // (knob off: P <= -1 never holds)
    for (;;) {
        // ---- wave 0 disposes of the searches that end at once: the free row's best cached column is unassigned and its
        // cache certifies that (no column settled, no price changes: the path is one edge) ----
        if (!PAR && w == 0) {
            // A pipeline over the free list (35 000 such searches at c3), three steps deep: while step k is decided, the prices of step
            // k + 1's cached columns, the cache row of step k + 2 and the position / row / length of step k + 3 are in flight --
            // prices do not change in this loop.  A STEP is a run of identical rows (ten slots per spot at c3: free together, identical
            // caches, consecutive in the free list; their lengths come from the whole-chip pass before the kernel, cl_rem): with the
            // prices fixed, the t-th row of the run takes the t-th lowest of the unassigned columns that tie at the minimum -- the whole
            // run is one step, and the step after it is known before this one is decided.  (Rounds 3-4 found a run's end inside the
            // step and started the pipeline again behind every run: four dependent loads per run, 1.5 us.)
            auto flush_one_edge = [&](int cnt) {
                if (lane < cnt) {
                    const int r = s.st_row[lane], cc = s.st_col[lane];
                    a.rowsol[r] = cc; a.colsol[cc] = r; a.cassign[cc] = s.st_val[lane];
                }
            };
            const int *remp = (a.same_prev && a.scx) ? cl_rem(a) : nullptr;
            int nst = 0;
            // stage 0: decided now; stage 1: cache row here, prices in flight; stage 2: row known, cache row in flight; stage 3: position
            // known, row and length in flight (as loaded: made uniform when the stage moves up)
            int p0, l0, r0, p1, l1, r1, p2, l2, r2, p3, l3v, r3v;
            uint32_t col0, col1, col2; float val0, val1, val2, vv0, vv1;
            auto start = [&](int ff) {                               // (cold: a chain of loads -- at the start and behind a run cut short)
                auto len_of = [&](int pp) -> int { return pp < numfree ? (remp ? uni(remp[pp]) : 1) : 1; };
                auto row_at = [&](int pp) -> int { return pp < numfree ? uni(a.freerows[pp]) : -1; };
                p0 = ff; l0 = len_of(p0); r0 = row_at(p0);
                p1 = p0 + l0; l1 = len_of(p1); r1 = row_at(p1);
                p2 = p1 + l1; l2 = len_of(p2); r2 = row_at(p2);
                p3 = p2 + l2; l3v = p3 < numfree ? (remp ? remp[p3] : 1) : 1; r3v = p3 < numfree ? a.freerows[p3] : -1;
                col0 = COLSENT; col1 = COLSENT; col2 = COLSENT; val0 = 0.0f; val1 = 0.0f; val2 = 0.0f;
                if (r0 >= 0) { col0 = a.cache_col[(int64_t)r0 * KC + lane]; val0 = a.cache_val[(int64_t)r0 * KC + lane]; }
                if (r1 >= 0) { col1 = a.cache_col[(int64_t)r1 * KC + lane]; val1 = a.cache_val[(int64_t)r1 * KC + lane]; }
                if (r2 >= 0) { col2 = a.cache_col[(int64_t)r2 * KC + lane]; val2 = a.cache_val[(int64_t)r2 * KC + lane]; }
                vv0 = (r0 >= 0 && lane < KCU && col0 != COLSENT) ? getv((int)col0) : 0.0f;
                vv1 = (r1 >= 0 && lane < KCU && col1 != COLSENT) ? getv((int)col1) : 0.0f;
            };
            start(f);
            while (f < numfree) {
                const int fr = r0, L = l0 < 1 ? 1 : l0;
                const uint32_t col = col0;
                const float val = val0, vv = vv0;
                // the stages move up (as if this step took its whole run: else the pipeline starts again below)
                const int n_p3 = p3, n_l3 = uni(l3v), n_r3 = uni(r3v);          // stage 3's row and length have arrived
                p0 = p1; l0 = l1; r0 = r1; col0 = col1; val0 = val1; vv0 = vv1;
                p1 = p2; l1 = l2; r1 = r2; col1 = col2; val1 = val2;
                vv1 = (r1 >= 0 && lane < KCU && col1 != COLSENT) ? getv((int)col1) : 0.0f;
                p2 = n_p3; l2 = n_l3 < 1 ? 1 : n_l3; r2 = n_r3;
                col2 = COLSENT; val2 = 0.0f;
                if (r2 >= 0) { col2 = a.cache_col[(int64_t)r2 * KC + lane]; val2 = a.cache_val[(int64_t)r2 * KC + lane]; }
                p3 = p2 + l2;
                l3v = p3 < numfree ? (remp ? remp[p3] : 1) : 1; r3v = p3 < numfree ? a.freerows[p3] : -1;
                const float tau = rdlane(val, KCU);
                const bool valid = lane < KCU && col != COLSENT;
                const uint32_t od = valid ? f2ord(val - vv) : 0xFFFFFFFFu;
                const uint32_t omin = wave_min_u32(od);
                const bool un = valid && od == omin && !is_asg((int)col);
                const uint64_t mu = __ballot(un);
                if (!(omin != 0xFFFFFFFFu && mu && tau > ord2f(omin))) break;
                // this row and the identical free rows right behind it, as many as there are tied unassigned columns
                const int cntmu = __popcll(mu);
                const int m = L < cntmu ? L : cntmu;
                if (nst + m > 64) { flush_one_edge(nst); nst = 0; }
                const int rank = __popcll(mu & lanemask_lt());           // cache rows are sorted by column: ranks go by column
                if (un && rank < m) {
                    // (no global store in the loop: a load is only returned after the stores issued before it are acknowledged, so
                    //  three stores per search made every search wait for the previous one's)
                    s.st_row[nst + rank] = fr + rank; s.st_col[nst + rank] = (int)col; s.st_val[nst + rank] = val;
                    if (CLDS) s_cs[col] = (uint16_t)(fr + rank);
                    atomicOr(&asg[col >> 5], 1u << (col & 31));
                }
                c_trivial += m; c_hops += m;
                f += m;
                nst += m;
                if (nst == 64) { flush_one_edge(nst); nst = 0; }
                if (m != L && f < numfree) start(f);                     // (the run's other rows are not one-edge searches: most likely the loop ends with the next step)
            }
            flush_one_edge(nst);
            if (lane == 0) {
                s.f = f;
                if (seg_done > 0 && f < numfree) {               // back to the driver?  (never before one search is done)
                    bool stop = a.aug_seg > 0 && seg_done >= a.aug_seg;
                    if (a.aug_seg == 0) {
                        if (s.waste >= a.aug_waste) { stop = true; if (!announced && a.seg_sync) atomicAdd(a.seg_sync, 1); announced = true; }
                        else if (a.seg_sync && a.seg_quorum > 0 && ld_sc1(a.seg_sync) >= a.seg_quorum) stop = true;
                    }
                    if (stop) s.stop = 1;
                }
            }
        }
        __syncthreads();
        AUG_LAP(t_triv)
        if (PAR) {
            if (fbase >= numfree || perr) break;                 // (the same decision in every workgroup)
            f = fbase + g;
        } else {
            f = uni(s.f);
            if (f >= numfree || uni(s.stop)) break;
        }
        const bool active = !PAR || f < numfree;                  // (PAR: the last batch may have fewer searches than workgroups)
        seg_done++;
        const int fr = a.freerows[active ? f : 0];
        const float *__restrict__ frow = a.cost + wrow_off(a.rowmap, fr, a.ld);
        const float ftau = a.cache_val[(int64_t)fr * KC + KCU];

        if (active) {
        // ---- root: d[j] = c[fr][j] - v[j] for the cached columns (pred = fr) ----
        if (w == 0) {
            const uint32_t col = a.cache_col[(int64_t)fr * KC + lane];
            const float val = a.cache_val[(int64_t)fr * KC + lane];
            if (EMB) {
                const float red = ld_sc1(a.cache_red + (int64_t)fr * KC + lane);
                if (lane < KCU && col != COLSENT) relax_to((int)col, (unsigned long long)f2ord(red) << 12, fr);
            } else if (lane < KCU && col != COLSENT) relax_to((int)col, (unsigned long long)f2ord(val - getv((int)col)) << 12, fr);
        }
        __syncthreads();

        for (;;) {
            // ================= rounds until no wave finds work =================
            int nd = 0;                                              // full-row relaxations the last round queued (leaves the rounds for them)
            for (;;) {
                const unsigned long long Tlv = uni(lv_of(s.T));          // label value of the best unassigned column so far
                // the two best dirty columns among the wave's blocks (one key per lane: the smallest of the blocks it looks at)
                // How many waves take part in a round: a round is bound by the CU's instruction issue (16 waves on 4 SIMDs: ~500
                // instructions each), so while the frontier is narrow -- shallow searches, the first and last rounds of deep ones --
                // four waves (one per SIMD, eight settlements at most) make a round several times shorter.  Block b belongs to wave
                // b mod W in this round; which wave settles what is a matter of efficiency only.
                const int W = wact;
                if (w >= W && rb[0] < 0 && rb[1] < 0) {              // nothing to pick from, no minimum to rebuild: straight to the barrier
                    __syncthreads();
                    const int any0 = uni(s.any[ph]), npd0 = uni(s.npk[ph]), np0 = npd0 & 0xFFFF;
                    ph = (ph + 1) % 3;
                    c_rounds++;
                    wact = np0 > 6 ? WNW : 4;
                    nd = PAR && (npd0 & AUG_ABORT) ? -1 : npd0 >> 16;        // (-1: the search is aborted)
                    if (!any0 || nd) break;
                    continue;
                }
                unsigned long long mk = ~0ull;
                if (w < W) for (int b = w + W * lane; b < nblk; b += W * 64) mk = umin64(mk, bmin[b]);
                // Which dirty column a wave settles next is a matter of efficiency only (any schedule reaches the same labels), what
                // must be exact is WHETHER a block holds work: a lane is eligible if its best key is below the best unassigned
                // column's label; among the eligible lanes the smallest distance goes first (one 32-bit reduction and a ballot per
                // pick -- the tight-hop counts do not order the picks).
                bool pk[AP]; int pj[AP], oi[AP];
                unsigned long long lab[AP];
                float ca[AP], vp[AP], val[AP];
                uint32_t col[AP];
                {
                    uint32_t dk = lv_of(mk) < Tlv ? (uint32_t)(mk >> 32) : 0xFFFFFFFFu;
#pragma unroll
                    for (int q = 0; q < AP; q++) {
                        const uint32_t m = wave_min_u32(dk);
                        pk[q] = m != 0xFFFFFFFFu;
                        const int l = pk[q] ? __ffsll((unsigned long long)__ballot(dk == m)) - 1 : 0;
                        pj[q] = (int)(rdlane((uint32_t)mk, l) & 0xFFFFFu);
                        if (lane == l) dk = 0xFFFFFFFFu;
                    }
                }
#pragma unroll
                for (int q = 0; q < AP; q++) {
                    // (the block's minimum is void from here on; it is rebuilt in the NEXT round, see below)
                    if (pk[q] && lane == 0) { atomicAnd(&dirty[pj[q] >> 5], ~(1u << (pj[q] & 31))); bmin[pj[q] >> 6] = ~0ull; }
                }
                if (lane == 0 && (pk[0] || pk[1] || rb[0] >= 0 || rb[1] >= 0)) { s.any[ph] = 1; if (pk[0]) atomicAdd(&s.npk[ph], (int)pk[0] + (int)pk[1]); }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          // the bits are cleared before the labels are read
                // Everything the two settlements read is requested in ONE go, without a branch in between: label and owner entry of
                // both columns, then (the owners come from LDS) both cache rows -- a wave without a pick reads column 0's, harmlessly.
                // (With the loads inside `if (picked)` blocks the compiler drains the memory counter at every join: label 0, label 1,
                //  cache rows, offer 0, offer 1 were five L2 round trips in a row, most of a round's 4.1 us.)
                int pjx[AP];
                unsigned long long lab_r[AP];
                float ca_r[AP], vp_r[AP];
                int oi_r[AP];
#pragma unroll
                for (int q = 0; q < AP; q++) {
                    pjx[q] = pk[q] ? pj[q] : 0;
                    lab_r[q] = ld_sc1(lbl + pjx[q]); ca_r[q] = ld_sc1(a.cassign + pjx[q]);
                }
                int p_r = PAR_GMAX + 1;                              // (the batch's P: in flight with the labels, looked at behind them)
                if (PAR && w == 0) p_r = ld_sc1(&pc->P[batchno & 1]);
                // ... and with them the labels of the dirty columns of the blocks the wave took from in the LAST round: the new
                // minimum of such a block is not on any round's critical path this way (it used to be a third round trip, behind a
                // second barrier).  Safe against the offers that go on meanwhile: the minimum was voided at the pick (store), the
                // dirty bits are read here, the labels after them, the result is merged with an atomic min -- an offer either set
                // its dirty bit before this read (then its label, completed before the bit, is seen) or lowers the minimum itself
                // after the void store.  The block yields no pick for one round; no round ends the search while a rebuild is due.
                // (When the number of waves taking part changes between two rounds -- 4 <-> 16 -- a block's NEW owner may pick from it in the very
                //  round its old owner's rebuild is merged: the rebuild can then put back a column that is being settled.  Labels are a
                //  fixed point, so results do not depend on it; the column is settled once more, which is why wide_aug_rounds and
                //  wide_aug_settled -- and nothing else -- may differ from run to run by a few units.)
                bool db[AP]; unsigned long long lbr[AP];
#pragma unroll
                for (int q = 0; q < AP; q++) {
                    const int c = (rb[q] < 0 ? 0 : rb[q]) * 64 + lane;
                    db[q] = rb[q] >= 0 && c < n && ((dirty[c >> 5] >> (c & 31)) & 1u);
                    lbr[q] = ld_sc1(lbl + (db[q] ? c : pjx[q]));
                }
#pragma unroll
                for (int q = 0; q < AP; q++) { vp_r[q] = getv(pjx[q]); oi_r[q] = getcs(pjx[q]); }
#pragma unroll
                for (int q = 0; q < AP; q++) {
                    oi[q] = uni(oi_r[q]);
                    const int oix = oi[q] < 0 ? 0 : oi[q];
                    col[q] = a.cache_col[(int64_t)oix * KC + lane];
                    // (EMB: the entry less its column's price, as of the last commit that changed it -- other workgroups write it between batches)
                    val[q] = EMB ? ld_sc1(a.cache_red + (int64_t)oix * KC + lane) : a.cache_val[(int64_t)oix * KC + lane];
                }
#pragma unroll
                for (int q = 0; q < AP; q++) {
                    lab[q] = pk[q] ? uni(lab_r[q]) : ~0ull; ca[q] = uni(ca_r[q]); vp[q] = uni(vp_r[q]);
                    if (!pk[q]) { col[q] = COLSENT; oi[q] = 0; }
                }
                if (PAR && w == 0 && uni(p_r) <= gthr && lane == 0) atomicOr(&s.npk[ph], AUG_ABORT);
                unsigned long long old[AP], co[AP];
                bool off[AP], dn[AP];
                float vc[AP];
#pragma unroll
                for (int q = 0; q < AP; q++) {                       // (the cached columns' prices: LDS, or one more request for both)
                    const bool valid = lane < KCU && col[q] != COLSENT;
                    vc[q] = EMB ? 0.0f : getv(valid ? (int)col[q] : pjx[q]);
                }
#pragma unroll
                for (int q = 0; q < AP; q++) {
                    off[q] = false; dn[q] = false; old[q] = 0; co[q] = 0;
                    const uint32_t dord = (uint32_t)(lab[q] >> 32), kq = (uint32_t)(lab[q] >> 20) & LKMAX;
                    if (pk[q] && lv_of(lab[q]) < Tlv) {
                        c_proc++;
                        if ((dense[oi[q] >> 5] >> (oi[q] & 31)) & 1u) { dn[q] = true; continue; }
                        const float h = (ca[q] - vp[q]) - ord2f(dord);
                        const unsigned long long lv = edge_lv(f2ord(EMB ? val[q] - h : (val[q] - vc[q]) - h), dord, kq);
                        off[q] = lane < KCU && col[q] != COLSENT && (int)col[q] != pj[q] && lv <= Tlv;
                        co[q] = lv;
                    }
                }
                {   // both columns' offers (a returning atomic min per lane that has one) in flight together: the lanes are masked by
                    // hand -- as two `if` blocks each atomic was followed by a full wait at the block's end
                    static_assert(AP == 2, "two offers per wave and round");
                    const uint64_t m0 = __ballot(off[0]), m1 = __ballot(off[1]);
                    if (m0 | m1) {
                        unsigned long long *p0 = lbl + (off[0] ? (int)col[0] : 0), *p1 = lbl + (off[1] ? (int)col[1] : 0);
                        const unsigned long long k0 = lkey(co[0], (uint32_t)oi[0]), k1 = lkey(co[1], (uint32_t)oi[1]);
                        unsigned long long r0, r1;
                        uint64_t sv;
                        asm volatile("s_mov_b64 %[sv], exec\n\t"
                                     "s_and_b64 exec, %[sv], %[m0]\n\t"
                                     "global_atomic_umin_x2 %[r0], %[a0], %[d0], off sc0\n\t"
                                     "s_and_b64 exec, %[sv], %[m1]\n\t"
                                     "global_atomic_umin_x2 %[r1], %[a1], %[d1], off sc0\n\t"
                                     "s_mov_b64 exec, %[sv]\n\t"
                                     "s_waitcnt vmcnt(0)"
                                     : [r0] "=&v"(r0), [r1] "=&v"(r1), [sv] "=&s"(sv)
                                     : [a0] "v"(p0), [d0] "v"(k0), [a1] "v"(p1), [d1] "v"(k1), [m0] "s"(m0), [m1] "s"(m1)
                                     : "memory");
                        old[0] = off[0] ? r0 : 0; old[1] = off[1] ? r1 : 0;
                    }
                }
#pragma unroll
                for (int q = 0; q < AP; q++) {
                    const bool better = off[q] && (lkey(co[q], (uint32_t)oi[q]) < old[q]);
                    if (__ballot(better) && better) after_offer((int)col[q], co[q], oi[q], old[q]);
                }
#pragma unroll
                for (int q = 0; q < AP; q++) {
                    if (!dn[q]) continue;                          // the owner's cache could not certify: its whole cost row
                    const uint32_t dord = (uint32_t)(lab[q] >> 32), kq = (uint32_t)(lab[q] >> 20) & LKMAX;
                    const float h = (ca[q] - vp[q]) - ord2f(dord);
                    if (n >= COOP_MIN_N) {                         // a long row: by the whole workgroup, behind the round's barrier (coop_dense_rows)
                        if (lane == 0) {
                            const int e = (atomicAdd(&s.npk[ph], 1 << 16) >> 16) & 0x3FFF;     // (AUG_ABORT may be set above the count)
                            s.st_row[e] = oi[q]; s.st_row[32 + e] = pj[q]; s.st_col[e] = (int)dord; s.st_col[32 + e] = (int)kq; s.st_val[e] = h;
                        }
                    } else {
                        const float *__restrict__ row = a.cost + wrow_off(a.rowmap, oi[q], a.ld);
                        const int pjq = pj[q], oiq = oi[q];
                        // (a full row offers hundreds of candidates below the best unassigned distance when many columns are near-equal:
                        //  the label is read first -- a plain L2 load -- and the atomic follows only where it would change something)
                        wave_row_sweep(row, n, lane, [&](int c, float x) {
                            const unsigned long long lv = edge_lv(f2ord((x - getv(c)) - h), dord, kq);
                            if (c != pjq && lv <= lv_of(s.T) && (lkey(lv, (uint32_t)oiq) < ld_sc1(lbl + c))) relax_to(c, lv, oiq);
                        });
                    }
                    c_dense++;
                    if (lane == 0) atomicAdd(&s.waste, 1);
                }
#pragma unroll
                for (int q = 0; q < AP; q++) {                       // last round's blocks: smallest (distance, k) among their dirty columns
                    if (rb[q] >= 0) {
                        const int c = rb[q] * 64 + lane;
                        // (the smallest distance with hop count 0 and one of its columns: a lower bound of the block's smallest label
                        //  is all a minimum has to be -- a pick re-reads the label)
                        const uint32_t dk = db[q] ? (uint32_t)(lbr[q] >> 32) : 0xFFFFFFFFu;
                        const uint32_t m = wave_min_u32(dk);
                        if (m != 0xFFFFFFFFu) {
                            const int l = __ffsll((unsigned long long)__ballot(dk == m)) - 1;
                            if (lane == 0) atomicMin(&bmin[rb[q]], ((unsigned long long)m << 32) | (uint32_t)(c - lane + l));
                        }
                    }
                    rb[q] = pk[q] ? (pj[q] >> 6) : -1;
                }
                __syncthreads();
                const int any = uni(s.any[ph]), npd = uni(s.npk[ph]), np = npd & 0xFFFF;     // picks of the round | full rows it queued << 16
                if (tid == 0) { s.any[(ph + 2) % 3] = 0; s.npk[(ph + 2) % 3] = 0; }   // (last read before this barrier, next set after the next one)
                ph = (ph + 1) % 3;
                c_rounds++;
                wact = np > 6 ? WNW : 4;
                nd = PAR && (npd & AUG_ABORT) ? -1 : npd >> 16;
                if (!any || nd) break;
            }
            if (PAR && nd < 0) {                                     // aborted: what the round queued is dropped with the search
                AUG_LAP(t_rounds)
                if (tid == 0) s.ab = 1;
                __syncthreads();                                     // (search_end reads it)
                break;
            }
            if (nd) {                                              // (outside the round loop: its code must not weigh on the rounds)
                coop_dense_rows<VLDS>(&s, nd, a.cost, a.rowmap, a.ld, n, w, lane, lbl, tch, dirty, bmin, asg, s_v, a.v);
                continue;
            }
            // ================= converged: do the caches certify what was skipped? =================
            AUG_LAP(t_rounds)
            const unsigned long long Tk = s.T;
            const uint32_t Dord = (uint32_t)(Tk >> 32);
            const float D = Tk == ~0ull ? INFINITY : ord2f(Dord);
            const int nt = s.ntouch;
            for (int q = tid; q < nt; q += WT) {
                const int k = ld_sc1(tch + q);
                const unsigned long long lbk = ld_sc1(lbl + k);
                const uint32_t dord = (uint32_t)(lbk >> 32);
                // every settled column: label below the end's -- also at the end's DISTANCE with fewer tight hops: an uncached
                // tight edge out of such a column would give (distance, k + 1), possibly below the end's label
                if (lv_of(lbk) < lv_of(Tk) && is_asg(k)) {
                    const int i = getcs(k);
                    if (!((dense[i >> 5] >> (i & 31)) & 1u)) {
                        const float h = (ld_sc1(a.cassign + k) - getv(k)) - ord2f(dord);
                        const float bound = a.cache_val[(int64_t)i * KC + KCU] - h;
                        if (!(bound > D)) {
                            atomicOr(&dense[i >> 5], 1u << (i & 31));
                            atomicOr(&dirty[k >> 5], 1u << (k & 31));
                            atomicMin(&bmin[k >> 6], lkey(lv_of(lbk), (uint32_t)k));
                            atomicAdd(&s.fail, 1);
                        }
                    }
                }
            }
            if (tid == 0 && !s.rootdense && !(ftau > D)) { s.rootdense = 1; s.doroot = 1; atomicAdd(&s.fail, 1); }
            c_verify++;
            __syncthreads();
            const int fail = s.fail;
            if (s.doroot)
                for (int c = tid; c < n; c += WT) {
                    const unsigned long long lv = (unsigned long long)f2ord(frow[c] - getv(c)) << 12;
                    if (lv <= lv_of(s.T) && (lkey(lv, (uint32_t)fr) < ld_sc1(lbl + c))) relax_to(c, lv, fr);
                }
            __syncthreads();
            if (tid == 0) { if (fail) s.anydense = 1; s.fail = 0; s.doroot = 0; }
            __syncthreads();
            AUG_LAP(t_verify)
            if (!fail) break;
        }

        }   // (active)

        // ---- the search has ended at s.T: [PAR: claim, find the conflict-free prefix of the batch;] price update, path flip, reset ----
        const unsigned long long Tk = active ? s.T : ~0ull;
        if (!PAR && Tk == ~0ull) { if (tid == 0) s.err = 1; __syncthreads(); break; }
        // (search_end, out of line; PAR: it meets the launch at one grid barrier)
        const unsigned long long er = uni(search_end<VLDS, CLDS, PAR>(batch, (lds_aug_t *)&s, (lds_u64_t *)w_smem, g, fr, batchno, pgen, active ? 1 : 0));
        if (PAR) pgen++;
        if (PAR && ((er >> 49) & 1)) {                            // aborted: the rounds were left in mid-flight -- no rebuild is due, the round flags start clean
#pragma unroll
            for (int q = 0; q < AP; q++) rb[q] = -1;
            wact = 4;
            if (tid == 0) { s.any[0] = 0; s.any[1] = 0; s.any[2] = 0; s.npk[0] = 0; s.npk[1] = 0; s.npk[2] = 0; s.ab = 0; s.nab++; }
        }
        const bool commit = (er >> 48) & 1;
        const int Pb = (int)((er >> 32) & 0xFFFFu);
        const int par = batchno & 1;
        c_hops += (long long)(uint32_t)er;
        if (PAR && active && !commit) c_discarded++;
        if (tid == 0) { if (commit) c_relax += s.scans; s.scans = 0; s.T = ~0ull; s.ntouch = 0; s.nset = 0; s.anydense = 0; s.rootdense = 0; s.f = f + 1; }
        f++;
        __syncthreads();
#ifdef CYTO_AUG_FIN_SPLIT
        if (PAR && tid == 0) fs_mark = wall_clock64();
#endif
        if (PAR) {
            // the batch's changes, into this workgroup's copies (its own included: harmless); then the next batch
            par_barrier(pc, G, pgen);
            perr = uni(ld_sc1(&pc->err));
            const int npl = uni(ld_sc1(&pc->nplog[par])), nol = uni(ld_sc1(&pc->nolog[par]));
            if (VLDS) for (int e = tid; e < npl; e += WT) s_v[ld_sc1(plog_col + e)] = ld_sc1(plog_val + e);
            for (int e = tid; e < nol; e += WT) {
                const int col = ld_sc1(olog_col + e);
                if (CLDS) s_cs[col] = (uint16_t)ld_sc1(olog_own + e);
                atomicOr(&asg[col >> 5], 1u << (col & 31));
            }
            __syncthreads();
            FS_LAP(FS_WAIT3)
            const int left = numfree - fbase;
            fbase += Pb < left ? Pb : left;                       // (Pb >= 1: the first search of a batch never conflicts)
            if (Pb < 1) perr = 1;
            if (EMB) {
                // the batch's price changes into cache_red, by every wave of every workgroup of the launch: eight log entries per wave
                // and step, the lanes over the repriced columns' lists (embed_repair); then the launch meets once more
                // (by the committing workgroup alone, before the third barrier: 64 scattered lines per store instruction from ONE CU,
                //  and a deep search's columns on its 16 waves -- update + flip + reset 7.0 -> 7.9 ms at 50 000^2)
                for (int e0 = (g * WNW + w) * 8; e0 < npl; e0 += G * WNW * 8) {
                    const bool have_e = lane < 8 && e0 + lane < npl;
                    const int k = have_e ? ld_sc1(plog_col + e0 + lane) : 0;
                    const float nv = have_e ? ld_sc1(plog_val + e0 + lane) : 0.0f;
                    embed_repair((gf32_t *)a.cache_red, (gci32_t *)a.inv_off, (gcu64_t *)a.inv_ent, __ballot(have_e), k, nv);
                }
                par_barrier(pc, G, pgen);
            }
            FS_LAP(FS_REPAIR)
#ifdef CYTO_AUG_FIN_SPLIT
            FS_SET(FS_SETTLED, s.st_col[63])
            if (tid == 0) s.st_col[63] = 0;
#endif
            batchno++; c_batches++;
        }
        AUG_LAP(t_finish)
    }

    // ---- duals, total, counters ----
    __syncthreads();
    __shared__ double s_tot[WNW];
    __shared__ long long s_wc[WNW][4];
    if (lane == 0) { s_wc[w][0] = c_proc; s_wc[w][1] = c_dense; s_wc[w][2] = c_trivial; s_wc[w][3] = (w == 0) ? c_hops : 0; }
    __syncthreads();
    long long proc = 0, dn = 0, triv = 0, hops0 = 0;
    for (int k = 0; k < WNW; k++) { proc += s_wc[k][0]; dn += s_wc[k][1]; triv += s_wc[k][2]; hops0 += s_wc[k][3]; }
    if (PAR) {                                                   // the workgroups' counters meet in the control block; workgroup 0 finishes
        if (tid == 0) {
            atomicAdd(reinterpret_cast<unsigned long long *>(&pc->c_relax), (unsigned long long)c_relax);
            atomicAdd(reinterpret_cast<unsigned long long *>(&pc->c_hops), (unsigned long long)hops0);
            atomicAdd(reinterpret_cast<unsigned long long *>(&pc->c_proc), (unsigned long long)proc);
            atomicAdd(reinterpret_cast<unsigned long long *>(&pc->c_dense), (unsigned long long)dn);
            atomicAdd(reinterpret_cast<unsigned long long *>(&pc->c_discarded), (unsigned long long)c_discarded);
            if (s.nab) atomicAdd(reinterpret_cast<unsigned long long *>(&pc->c_aborted), (unsigned long long)s.nab);
            if (g == 0) { pc->c_rounds = c_rounds; pc->c_verify = c_verify; pc->c_batches = c_batches; }
        }
        par_barrier(pc, G, pgen);
        if (g != 0) return;
        c_relax = (long long)ld_sc1(reinterpret_cast<unsigned long long *>(&pc->c_relax));
        hops0 = (long long)ld_sc1(reinterpret_cast<unsigned long long *>(&pc->c_hops));
        proc = (long long)ld_sc1(reinterpret_cast<unsigned long long *>(&pc->c_proc));
        dn = (long long)ld_sc1(reinterpret_cast<unsigned long long *>(&pc->c_dense));
        f = perr || ld_sc1(&pc->err) ? f : numfree;
    }
    double tot = 0.0;
    for (int i = tid; i < n; i += WT) {
        const int j = ld_sc1(a.rowsol + i);
        if (j >= 0) {
            const float cij = ld_sc1(a.cassign + j);
            a.u[i] = cij - ld_sc1(a.v + j);
            tot += (double)cij;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) tot += __shfl_xor(tot, off);
    if (lane == 0) s_tot[w] = tot;
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        for (int k = 0; k < WNW; k++) t += s_tot[k];
        const bool err = s.err || (PAR && (perr || ld_sc1(&pc->err)));
        LapStatus *st = lap_status(a.misc);
        st->total = t;
        long long *ctr = st->counters, *wc = st->wide;
        ctr[C_AUG_INIT] = numfree; ctr[C_AUG_RELAX] += c_relax; ctr[C_AUGS] = numfree; ctr[C_HOPS] += hops0;
        wc[WC_DENSE_AUG] += dn; wc[WC_AUG_LAUNCHES] += 1; wc[WC_AUG_ROUNDS] += c_rounds; wc[WC_AUG_PROCESSED] += proc; wc[WC_TRIVIAL] += triv; wc[WC_VERIFY_PASSES] += c_verify;
        if (err) st->status = 1;
        st->wide_done = err ? numfree : f;      // searches done (an error ends them)
        if (a.seg_sync) a.seg_sync[1 + (PAR ? 0 : blockIdx.x)] = err ? 0 : numfree - f;
        long long *tmr = st->timers;
        tmr[WT_AUG_ROUNDS_TICKS] += t_rounds; tmr[WT_AUG_VERIFY_TICKS] += t_verify; tmr[WT_AUG_FINISH_TICKS] += t_finish; tmr[WT_AUG_TRIVIAL_TICKS] += t_triv;
        if (PAR) st->wide_embedded = EMB ? 1 : 0;
        if (PAR) st->wide_aborted = (int)ld_sc1(reinterpret_cast<unsigned long long *>(&pc->c_aborted));
        if (PAR) { tmr[WT_PAR_BATCHES] = ld_sc1(reinterpret_cast<unsigned long long *>(&pc->c_batches)); tmr[WT_PAR_DISCARDED] = ld_sc1(reinterpret_cast<unsigned long long *>(&pc->c_discarded)); }
    }
}

// ------------------------------------------------------------------------------------------------------------------
// ------------------------------------------------------------------------------------------------------------------
// ONE-EDGE SEARCHES ON THE WHOLE CHIP (CytoSPACE's repeated spot rows: reference linear_assignment_solvers.py:61-66 expands a spot into one
// identical row per slot; at config c3 35 000 of the 50 000 rows reach the searches and every one of their searches is a single edge).
// wide_aug's wave 0 disposes of such searches one after the other -- the free row's cache certifies its minimum, a column tied at that
// minimum is unassigned: the row takes the lowest such column, no price changes -- 0.22 us per row in runs, 7.7 ms at c3.  With the
// prices fixed that loop is a SERIAL DICTATORSHIP: row after row, in free-list order, takes the first column of a fixed list (its cached
// columns tied at its minimum, by column) that nobody before it took, and the loop ends at the first row that finds none.  Deferred
// acceptance computes the same assignment in parallel: every row proposes down its list, a column keeps the EARLIEST row that ever
// proposed (an atomic min of free-list positions -- claims only improve, so a column lost to an earlier row is lost for good), a row
// that lost its column moves on; at the fixed point the rows before the first one that ran out of columns hold exactly what the serial
// loop gives them (a later row never takes anything from an earlier one), and those are committed; wide_aug starts behind them.  The
// t-th row of a run of identical rows starts at its list's t-th column (the t rows before it want the same columns and come first).
// Scratch: the machine's arrays (a.scx; the row reduction is over): claims [n], lists as lane masks [n], {next candidate, lane held} [n].
// ------------------------------------------------------------------------------------------------------------------
// the k-th set bit of m at or after ... : lane of the (k + 1)-th set bit, -1 if there are not that many
__device__ __forceinline__ int nth_set(unsigned long long m, int k) {
    for (int t = 0; t < k && m; t++) m &= m - 1;
    return m ? __ffsll((long long)m) - 1 : -1;
}

// a wave per free row: its list (the cached columns tied at the row's minimum and unassigned, as a lane mask -- cache rows are sorted by
// column; 0: the cache does not certify the minimum, or nothing is free: the serial loop would stop here) and where it starts
__global__ __launch_bounds__(HEADB) void wide_claim_lists(const WideArgs *__restrict__ batch) {
    const WideArgs a = load_wide_args(batch, blockIdx.y);
    const int numfree = lap_status(a.misc)->numfree;
    const int lane = threadIdx.x & 63;
    const int gw = blockIdx.x * (HEADB / 64) + (threadIdx.x >> 6), nw = gridDim.x * (HEADB / 64);
    if (blockIdx.x == 0 && threadIdx.x == 0) { ClaimCtl *c = cl_ctl(a); c->changed = 0; c->blocked = 0x7FFFFFFF; c->rounds = 0; }
    for (int i = blockIdx.x * HEADB + threadIdx.x; i < a.n; i += gridDim.x * HEADB) cl_claim(a)[i] = 0x7FFFFFFF;
    for (int p = gw; p < numfree; p += nw) {
        const int fr = uni(a.freerows[p]);
        const uint32_t col = a.cache_col[(int64_t)fr * KC + lane];
        const float val = a.cache_val[(int64_t)fr * KC + lane];
        const float tau = rdlane(val, KCU);
        const bool valid = lane < KCU && col != COLSENT;
        const float vv = valid ? a.v[col] : 0.0f;
        const int ow = valid ? a.colsol[col] : 0;
        const uint32_t od = valid ? f2ord(val - vv) : 0xFFFFFFFFu;
        const uint32_t omin = wave_min_u32(od);
        unsigned long long mu = __ballot(valid && od == omin && ow < 0);
        if (!(omin != 0xFFFFFFFFu && tau > ord2f(omin))) mu = 0;
        if (lane == 0) {
            // rank in the run of identical rows this row belongs to (consecutive in the free list, each the copy of the row before it)
            int t = 0;
            if (a.same_prev)
                while (t < 63 && p - t - 1 >= 0 && a.same_prev[fr - t] != 0 && a.freerows[p - t - 1] == fr - t - 1) t++;
            cl_mask(a)[p] = mu;
            cl_state(a)[p] = make_int2(t, -1);                   // x: candidates of the list passed over so far; y: the lane it holds (-1: none, -2: ran out)
            if (t == 0) {                                        // the head of a run: its length, for wide_aug's loop over the rows left
                int len = 1;
                if (a.same_prev)
                    while (p + len < numfree && a.freerows[p + len] == fr + len && a.same_prev[fr + len] != 0) len++;      // (the position first: fr + len < n only while the list says so)
                for (int k = 0; k < len; k++) cl_rem(a)[p + k] = len - k;
            }
        }
    }
}

// a round: a thread per free row -- still holding its column?  else down the list to the next column no earlier row has
__global__ __launch_bounds__(HEADB) void wide_claim_round(const WideArgs *__restrict__ batch) {
    const WideArgs a = load_wide_args(batch, blockIdx.y);
    const int numfree = lap_status(a.misc)->numfree;
    int *claim = cl_claim(a);
    int changed = 0;
    for (int p = blockIdx.x * HEADB + threadIdx.x; p < numfree; p += gridDim.x * HEADB) {
        int2 st = cl_state(a)[p];
        if (st.y == -2) continue;
        const int fr = a.freerows[p];
        const unsigned long long m = cl_mask(a)[p];
        if (st.y >= 0) {
            if (claim[a.cache_col[(int64_t)fr * KC + st.y]] == p) continue;      // (still the earliest row that asked)
            st.x++; st.y = -1; changed = 1;
        }
        for (;;) {
            const int l = nth_set(m, st.x);
            if (l < 0) { st.y = -2; changed = 1; break; }
            const int c = (int)a.cache_col[(int64_t)fr * KC + l];
            if (claim[c] > p && atomicMin(claim + c, p) > p) { st.y = l; changed = 1; break; }
            st.x++;
        }
        cl_state(a)[p] = st;
    }
    if (__ballot(changed) && (threadIdx.x & 63) == 0) atomicAdd(&cl_ctl(a)->changed, 1);
}

// after a few rounds: did anything move?  One thread looks at every problem of the batch and reports into pinned host memory (no
// synchronisation: the driver polls) -- hs[0] = groups of rounds checked so far, hs[1] = the first group after which NO problem had
// moved (0: none yet; rounds at the fixed point change nothing, so the groups the driver queued ahead are harmless).
__global__ void wide_claim_check(const WideArgs *__restrict__ batch, int nb, int group, int *hs) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int any = 0;
    for (int b = 0; b < nb; b++) {
        const WideArgs a = load_wide_args(batch, b);
        ClaimCtl *c = cl_ctl(a);
        any |= c->changed;
        c->changed = 0; c->rounds += 1;
    }
    if (!any && __hip_atomic_load(hs + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == 0)
        __hip_atomic_store(hs + 1, group, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(hs, group, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// the fixed point: the first row that ran out of columns ...
__global__ __launch_bounds__(HEADB) void wide_claim_blocked(const WideArgs *__restrict__ batch) {
    const WideArgs a = load_wide_args(batch, blockIdx.y);
    const int numfree = lap_status(a.misc)->numfree;
    int first = 0x7FFFFFFF;
    for (int p = blockIdx.x * HEADB + threadIdx.x; p < numfree; p += gridDim.x * HEADB)
        if (cl_state(a)[p].y < 0) { first = p; break; }           // (positions ascend along a thread's stride: its first is its lowest)
    if (first != 0x7FFFFFFF) atomicMin(&cl_ctl(a)->blocked, first);
}
// ... and the rows before it take their columns: the serial loop's assignments (no price changes; one hop each)
__global__ __launch_bounds__(HEADB) void wide_claim_commit(const WideArgs *__restrict__ batch) {
    const WideArgs a = load_wide_args(batch, blockIdx.y);
    const int numfree = lap_status(a.misc)->numfree;
    const int pb = min(cl_ctl(a)->blocked, numfree);
    for (int p = blockIdx.x * HEADB + threadIdx.x; p < pb; p += gridDim.x * HEADB) {
        const int fr = a.freerows[p], l = cl_state(a)[p].y;
        const int c = (int)a.cache_col[(int64_t)fr * KC + l];
        a.rowsol[fr] = c; a.colsol[c] = fr; a.cassign[c] = a.cache_val[(int64_t)fr * KC + l];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        LapStatus *st = lap_status(a.misc);
        st->counters[C_HOPS] += pb; st->wide[WC_TRIVIAL] += pb;
        st->wide_done = pb;             // wide_aug starts behind them
    }
}

int wide_launch_claims(const WideArgs *d_args, int nb, int n, hipStream_t stream, int32_t *d_sync) {
    // the one-edge searches of every problem, on the whole chip (above); rounds in groups of four, then "did anything move?" -- reported
    // into pinned host memory: the driver keeps two groups queued ahead of the one under way and never waits for the stream
    if (n < 2 || !d_sync) return CYTO_OK;
    const int bxw = std::max(1, std::min((n + HEADB / 64 - 1) / (HEADB / 64), std::max(64, 4096 / std::max(1, nb))));
    const int bxt = std::max(1, std::min((n + HEADB - 1) / HEADB, std::max(16, 1024 / std::max(1, nb))));
    PinnedInts pin;
    int rc;
    if ((rc = pin.ensure(4, stream))) return rc;
    volatile int *hs = pin.p;
    hs[0] = 0; hs[1] = 0;
    hipLaunchKernelGGL(wide_claim_lists, dim3(bxw, nb), dim3(HEADB), 0, stream, d_args);
    constexpr int kAhead = 2, kMaxGroups = 1 << 16;
    int group = 0;
    SpinWait sw;
    auto t_progress = std::chrono::steady_clock::now();
    int seen = 0;
    bool fixed = false;
    for (;;) {
        if (hs[1] != 0) { fixed = true; break; }
        const int done = hs[0];
        if (done != seen) { seen = done; t_progress = std::chrono::steady_clock::now(); sw.reset(); }
        if (group - done >= kAhead) {
            sw.pause();
            if ((sw.polls & 0xFFFF) == 0) {
                const bool drained = hipStreamQuery(stream) != hipErrorNotReady;
                if ((drained && hs[0] == done && hs[1] == 0) ||                                   // (the queue has drained and nobody reported: a launch failed)
                    std::chrono::steady_clock::now() - t_progress > std::chrono::seconds(120)) {   // (no group finished for two minutes)
                    (void)hipStreamSynchronize(stream);
                    return CYTO_ERR_INTERNAL;
                }
            }
            continue;
        }
        if (group >= kMaxGroups) break;                                   // (a row moves down its list at most 63 times: cannot happen)
        group++;
        for (int k = 0; k < 4; k++) hipLaunchKernelGGL(wide_claim_round, dim3(bxt, nb), dim3(HEADB), 0, stream, d_args);
        hipLaunchKernelGGL(wide_claim_check, dim3(1), dim3(64), 0, stream, d_args, nb, group, pin.p);
    }
    if (!fixed) { (void)hipStreamSynchronize(stream); return CYTO_ERR_INTERNAL; }      // (never commit an assignment that is not the fixed point)
    hipLaunchKernelGGL(wide_claim_blocked, dim3(bxt, nb), dim3(HEADB), 0, stream, d_args);
    hipLaunchKernelGGL(wide_claim_commit, dim3(bxt, nb), dim3(HEADB), 0, stream, d_args);
    CYTO_HIP(hipGetLastError());
    return CYTO_OK;                                                       // (the pinned block: usable again behind the check kernels still queued)
}

// ---- the embedded form's arrays, built by the whole chip between the last cache build and the searches ----
// a wave per row: the entries less their columns' prices; every entry's rank in its column's list (which also counts the lists)
__global__ __launch_bounds__(256) void embed_red_count(int n, const uint32_t *__restrict__ cache_col, const float *__restrict__ cache_val,
                                                       const float *__restrict__ v, float *__restrict__ red, int32_t *__restrict__ cnt,
                                                       int32_t *__restrict__ rank) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const uint32_t col = cache_col[(int64_t)i * KC + lane];
    const float val = cache_val[(int64_t)i * KC + lane];
    const bool valid = lane < KCU && col < (uint32_t)n;
    red[(int64_t)i * KC + lane] = valid ? val - v[col] : 0.0f;
    if (valid) rank[(int64_t)i * KC + lane] = atomicAdd(cnt + col, 1);
}
// EMB_SB columns per workgroup: their counts' sum and maximum
__global__ __launch_bounds__(EMB_SB) void embed_block_sums(int n, const int32_t *__restrict__ cnt, int32_t *__restrict__ bsum) {
    __shared__ int ws[EMB_SB / 64], wm[EMB_SB / 64];
    const int j = blockIdx.x * EMB_SB + threadIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int c = j < n ? cnt[j] : 0, mx = c;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { c += __shfl_xor(c, d); mx = max(mx, __shfl_xor(mx, d)); }
    if (lane == 0) { ws[w] = c; wm[w] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0, m = 0;
        for (int k = 0; k < EMB_SB / 64; k++) { t += ws[k]; m = max(m, wm[k]); }
        bsum[blockIdx.x] = t; bsum[gridDim.x + blockIdx.x] = m;
    }
}
// list starts: the sums of the workgroups before this one (every workgroup adds them up for itself), then its own columns;
// workgroup 0 also leaves the total in off[n] and the longest list in cnt[n]
__global__ __launch_bounds__(EMB_SB) void embed_scan(int n, int32_t *__restrict__ cnt, const int32_t *__restrict__ bsum, int32_t *__restrict__ off) {
    __shared__ int ws[EMB_SB / 64], wm[EMB_SB / 64], wt[EMB_SB / 64];
    const int nb = gridDim.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int before = 0, total = 0, mx = 0;
    for (int k = tid; k < nb; k += EMB_SB) { const int t = bsum[k]; total += t; if (k < (int)blockIdx.x) before += t; mx = max(mx, bsum[nb + k]); }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { before += __shfl_xor(before, d); total += __shfl_xor(total, d); mx = max(mx, __shfl_xor(mx, d)); }
    if (lane == 0) { ws[w] = before; wt[w] = total; wm[w] = mx; }
    const int j = blockIdx.x * EMB_SB + tid;
    const int c = j < n ? cnt[j] : 0;
    int inc = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(inc, d); if (lane >= d) inc += t; }
    __shared__ int wi[EMB_SB / 64];
    if (lane == 63) wi[w] = inc;
    __syncthreads();
    int base = 0, tot = 0, m = 0;
    for (int k = 0; k < EMB_SB / 64; k++) { base += ws[k]; tot += wt[k]; m = max(m, wm[k]); if (k < w) base += wi[k]; }
    if (j < n) off[j] = base + inc - c;
    if (blockIdx.x == 0 && tid == 0) { off[n] = tot; cnt[n] = m; }
}
__global__ __launch_bounds__(256) void embed_fill(int n, const uint32_t *__restrict__ cache_col, const float *__restrict__ cache_val,
                                                  const int32_t *__restrict__ off, const int32_t *__restrict__ rank, unsigned long long *__restrict__ ent) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const uint32_t col = cache_col[(int64_t)i * KC + lane];
    const float val = cache_val[(int64_t)i * KC + lane];
    if (lane < KCU && col < (uint32_t)n)
        ent[off[col] + rank[(int64_t)i * KC + lane]] = ((unsigned long long)__float_as_uint(val) << 32) | ((uint32_t)i << 6) | (uint32_t)lane;
}
int wide_build_embedded(const WideArgs &wa, int n, hipStream_t stream) {
    char *eb = reinterpret_cast<char *>(wa.cache_red);
    int32_t *cnt = emb_counts(wa, n), *bsum = reinterpret_cast<int32_t *>(eb + emb_off_bsum(n)), *rank = reinterpret_cast<int32_t *>(eb + emb_off_rank(n));
    const int nb = emb_blocks(n);
    CYTO_HIP(hipMemsetAsync(cnt, 0, ((size_t)n + 1) * 4, stream));
    hipLaunchKernelGGL(embed_red_count, dim3((n + 3) / 4), dim3(256), 0, stream, n, wa.cache_col, wa.cache_val, wa.v, wa.cache_red, cnt, rank);
    hipLaunchKernelGGL(embed_block_sums, dim3(nb), dim3(EMB_SB), 0, stream, n, cnt, bsum);
    hipLaunchKernelGGL(embed_scan, dim3(nb), dim3(EMB_SB), 0, stream, n, cnt, bsum, const_cast<int32_t *>(wa.inv_off));
    hipLaunchKernelGGL(embed_fill, dim3((n + 3) / 4), dim3(256), 0, stream, n, wa.cache_col, wa.cache_val, wa.inv_off, rank, const_cast<unsigned long long *>(wa.inv_ent));
    CYTO_HIP(hipGetLastError());
    return CYTO_OK;
}

// which of the searches' arrays live in LDS
// (developer knob, read once per process: CYTO_AUG_LDS = 2 or unset: by size; 1: owners in LDS, prices global -- what n > ~24 000
//  gets; 0: neither -- the n > 65 534 instantiation.  It only takes arrays OUT of LDS: same results, tools/wide_large.py)
void wide_aug_lds_choice(int n, bool &vlds, bool &clds) {
    const int lds_knob = CYTO_KNOB("CYTO_AUG_LDS").set ? CYTO_KNOB("CYTO_AUG_LDS").value : 2;
    vlds = lds_knob >= 2 && wide_aug_vlds(n); clds = lds_knob >= 1 && wide_aug_clds(n);
}

int wide_launch_aug(const WideArgs *d_args, int nb, int n, hipStream_t stream, int par_groups, bool embed) {
    bool vlds, clds;
    wide_aug_lds_choice(n, vlds, clds);
    const size_t shm = wide_aug_lds_bytes(n, vlds, clds);
    if (shm > (size_t)LDS_DYNAMIC_MAX) return CYTO_ERR_UNSUPPORTED;
    if (par_groups > 1) {                                         // one problem, several SEARCHES at once (blocks 0, 8, 16 ... take part)
        void (*k)(const WideArgs *) = vlds ? wide_aug<true, true, true> : clds ? wide_aug<false, true, true> : wide_aug<false, false, true>;
        if (embed) {
            if (vlds) return CYTO_ERR_INTERNAL;
            k = clds ? wide_aug<false, true, true, true> : wide_aug<false, false, true, true>;
        }
        int rc = set_max_dynamic_lds(reinterpret_cast<const void *>(k));
        if (rc) return rc;
        // (the searches' workgroups spread over all XCDs -- each with its own labels in its own L2 -- instead of packed on one: wide_aug 9.01 ->
        //  8.84 ms at 20 000^2, 20.6 -> 20.1 at 50 000^2, gpurun_out/r05l; developer knob CYTO_PAR_STRIDE = 8: the one-XCD placement)
        const int pstride = CYTO_KNOB("CYTO_PAR_STRIDE").set ? std::max(1, CYTO_KNOB("CYTO_PAR_STRIDE").value) : 1;
        hipLaunchKernelGGL(k, dim3(pstride * par_groups), dim3(WT), shm, stream, d_args);
        CYTO_HIP(hipGetLastError());
        return CYTO_OK;
    }
    void (*k)(const WideArgs *) = vlds ? wide_aug<true, true, false> : clds ? wide_aug<false, true, false> : wide_aug<false, false, false>;
    int rc = set_max_dynamic_lds(reinterpret_cast<const void *>(k));
    if (rc) return rc;
    hipLaunchKernelGGL(k, dim3(nb), dim3(WT), shm, stream, d_args);
    CYTO_HIP(hipGetLastError());
    return CYTO_OK;
}
}  // namespace cyto

#ifdef CYTO_AUG_FIN_SPLIT
// the batch ends of the solves since the last call, by parts: out[batch][workgroup][part] in 100-MHz ticks (tools/fin_split.py); then cleared
extern "C" int cyto_wide_fin_split(long long *out, int *max_batches, int *groups, int *parts) {
    using namespace cyto;
    *max_batches = FS_MAXB; *groups = FS_G; *parts = FS_NP;
    if (!out) return 0;
    if (hipDeviceSynchronize() != hipSuccess) return 5;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_fs), sizeof(long long) * FS_MAXB * FS_G * FS_NP) != hipSuccess) return 5;
    void *p = nullptr;
    if (hipGetSymbolAddress(&p, HIP_SYMBOL(g_fs)) != hipSuccess || hipMemset(p, 0, sizeof(long long) * FS_MAXB * FS_G * FS_NP) != hipSuccess) return 5;
    return 0;
}
#endif
