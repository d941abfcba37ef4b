// lap_wide_rr.hip -- the wide solver's ROW-REDUCTION side (lap_wide.hip describes the solver and holds its searches; lap_wide_drv.hip is the host driver): the reduction transfer with the scale
// of the instance (wide_rt), the eps-scaled phase machine on the whole chip (wide_sc_*), the chain rounds and free lists (wide_arr),
// and the launches of all of these.
#include "lap_wide_dev.h"

namespace cyto {

namespace {

// Which of the 64 sorted lane minima of a row is tried first as the floor of its fresh cache.  The number of columns below the
// (k + 1)-th smallest lane minimum is the number of draws it takes to hit k + 1 of 64 lanes, less one (distribution-free when the
// values are distinct): k = 34 -> 49 +- 5 columns, more than 63 in 0.4 % of the rows; k = 47 (rounds 3-4) -> 86 +- 10: the first
// collecting sweep failed in 99.8 % of the rows and the second candidate (k = 23) left caches of 29 columns.
constexpr int SC_FLOOR_POS = 34;

}  // namespace

// ------------------------------------------------------------------------------------------------------------------
// The control block of the row-reduction phase (WideArgs.sc, 2 KB, zeroed by the driver): the scale of the instance that
// wide_rt measures, and the state of the phase machine below (wide_sc_*).
// ------------------------------------------------------------------------------------------------------------------
enum { SC_LEGACY = 0, SC_EPS = 1, SC_FINAL = 2, SC_HANDOVER = 3, SC_DONE = 4 };   // modes (>= SC_HANDOVER: the machine is through)
enum { SC_ACT_NONE = 0, SC_ACT_ROUND = 1, SC_ACT_RESET = 2 };                      // what a launch does
// `fresh`: the list launch L reads was made by wide_sc_init (rows that have not bid yet); else its rows bid in launch L - 1
struct ScSlot { int mode, k, rip, fresh, act; float eps; long long total, bids; int heavy, pad_; };   // heavy: the instance bids from full rows a lot (as of the launch before: the same for every workgroup)
struct ScRound { int cnt, retired; };   // per launch (three cells in rotation: L % 3): rows that bid in it, how many of them retired
struct ScCtl {
    int hist[256];                 // rows per binary exponent (the exponent FIELD) of their gap u2 - u1 at the post-column-reduction prices
    uint32_t vmaxbits;             // bits of max_j |v0[j]|
    int e0;                        // exponent field of eps_0 (0: the instance never scales)
    float epsmin;                  // phases end below this eps (the resolution of the prices)
    int stop;                      // WIDE_STOP(n)
    ScRound rnd[3];
    int retired, dense, dense_mark, phases, free_cr;
    int fin_buf, fin_cnt;          // where the machine stopped: the record buffer and the length of the list it leaves
    int want_mark, pad2_;          // the launch at which fresh row caches were last asked for
    unsigned long long wbase[2];   // per bid-word buffer: the launch at which it was last wiped (the words' 12-bit tag is relative to it)
    ScSlot slot[2];                // launch L reads slot[L & 1] and leaves slot[(L + 1) & 1]
};
static_assert(sizeof(ScCtl) <= 2048, "control block of the row-reduction phase");
// the constants of the restatement (oracle/jv_oracle.h: JV_WIDE_*)
constexpr int SC_K0 = 8, SC_NPH = 16, SC_PHCAP = 1024, SC_EMULT = 3, SC_ESTEP = 1;
constexpr int SC_STOP_FINAL = 16;       // the final eps = 0 phase ends at min(wide_stop(n), 16) active rows (JV_WIDE_STOP_FINAL)
constexpr int SC_UNROLL = 4;           // quads of a full-row sweep in flight per lane (2: 67 registers, 7 waves per SIMD; 3: 79, 6; 4: 107, 4 -- and 4 is the fastest: gpurun_out/r05h)
#ifndef HEAVY_SPREAD
#define HEAVY_SPREAD 1
#endif
constexpr int SC_SMALL = 2048;         // launches with at most so many bids to resolve give every bid a wave of its own (a matter of speed only)
constexpr int SC_COARSE = 4;           // phases whose full-row bids leave the row caches alone (a matter of speed only)
#ifndef WIDE_STOP_CAP
#define WIDE_STOP_CAP 64
#endif
__host__ __device__ inline int wide_stop(int n) { return n / 128 < 8 ? 8 : (n / 128 > WIDE_STOP_CAP ? WIDE_STOP_CAP : n / 128); }
// the next representable value below x (+0 and -0 are one value): oracle pred_
__device__ __forceinline__ float pred_f32(float x) {
    const uint32_t o = f2ord(x);
    float r = ord2f(o - 1u);
    if (!(r < x)) r = ord2f(o - 2u);
    return r;
}

// ------------------------------------------------------------------------------------------------------------------
// REDUCTION TRANSFER (Jacobi) -- and the scale of the instance.  v0 = the post-column-reduction prices (a copy lives in
// a.cassign, which also is the raw cost of every column's owner entry at that point: the column minimum).
// Every row takes the lexicographic top-2 (u1, j1), (u2, j2) of c[i][.] - v0[.]: its gap u2 - u1 goes into the histogram of
// binary exponents (integer counts: no order); a row that owns exactly one column jo subtracts its margin
//   v[jo] = v0[jo] - min_{j != jo} (c[i][j] - v0[j])        (= u2 if j1 == jo, else u1)
// The cache was built against v0: it holds EVERY column with c - v0 < floor, so a cached second minimum < floor is the row's.
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RTB) void wide_rt(const WideArgs *__restrict__ batch) {
    const WideArgs a = load_wide_args(batch, blockIdx.y);
    const int n = a.n;
    if (n < 2) return;
    __shared__ int s_hist[256];
    __shared__ uint32_t s_vmax;
    for (int e = threadIdx.x; e < 256; e += RTB) s_hist[e] = 0;
    if (threadIdx.x == 0) s_vmax = 0;
    __syncthreads();
    ScCtl *sc = reinterpret_cast<ScCtl *>(a.sc);
    const int lane = threadIdx.x & 63;
    const int gw = blockIdx.x * (RTB / 64) + (threadIdx.x >> 6), nw = gridDim.x * (RTB / 64);
    const float *__restrict__ v0 = a.cassign;
    {
        uint32_t m = 0;
        for (int j = blockIdx.x * RTB + threadIdx.x; j < n; j += gridDim.x * RTB) { const uint32_t x = __float_as_uint(fabsf(v0[j])); m = m > x ? m : x; }
        if (m) atomicMax(&s_vmax, m);
    }
    long long done = 0;
    for (int i = gw; i < n; i += nw) {
        const uint32_t col = a.cache_col[(int64_t)i * KC + lane];
        const float val = a.cache_val[(int64_t)i * KC + lane];
        const float tau = __shfl(val, KCU);
        const bool valid = lane < KCU && col != COLSENT;
        const uint32_t key = valid ? f2ord(val - v0[col]) : 0xFFFFFFFFu;
        const uint32_t k1 = wave_min_u32(key);
        const int l1 = __ffsll((unsigned long long)__ballot(key == k1)) - 1;
        const uint32_t k2 = wave_min_u32(lane == l1 ? 0xFFFFFFFFu : key);
        float u1, u2; int j1;
        if (k2 != 0xFFFFFFFFu && ord2f(k2) < tau) { u1 = ord2f(k1); u2 = ord2f(k2); j1 = (int)rdlane(col, l1); }
        else {                                                  // the cache cannot certify the top-2: the whole row
            const float *__restrict__ row = a.cost + wrow_off(a.rowmap, i, a.ld);
            K2 d; d.m1 = KEYMAX; d.m2 = KEYMAX;
            wave_row_sweep(row, n, lane, [&](int c, float x) { k2_push(d, mkkey(x - v0[c], (uint32_t)c)); });
            d = k2_wave_allreduce(d);
            u1 = key_val(d.m1); u2 = key_val(d.m2); j1 = (int)(uint32_t)d.m1;
        }
        if (lane == 0) atomicAdd(&s_hist[(__float_as_uint(u2 - u1) >> 23) & 0xFFu], 1);
        if (a.matches[i] == 1) {
            const int jo = a.rowsol[i];
            if (lane == 0) a.v[jo] = v0[jo] - (j1 == jo ? u2 : u1);
            done++;
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < 256; e += RTB) if (s_hist[e]) atomicAdd(&sc->hist[e], s_hist[e]);
    if (threadIdx.x == 0 && s_vmax) atomicMax(&sc->vmaxbits, s_vmax);
    if (lane == 0 && done) atomicAdd(reinterpret_cast<unsigned long long *>(lap_status(a.misc)->counters) + C_RT, (unsigned long long)done);
}

// ------------------------------------------------------------------------------------------------------------------
// AUGMENTING ROW REDUCTION, Jacobi rounds (oracle/jv_oracle_impl.h, wide mode).  One workgroup per problem.
//
// VLDS: the prices (f32) and the column owners (u16, 0xFFFF = unassigned) live in LDS beside their global copies (every
// update goes to both), so a bid is: the row's cache (two coalesced 256-B loads), 63 LDS gathers, two DPP reductions, two
// LDS look-ups.  Otherwise (n > ~26 000) both stay in L2 and are read with agent-scope loads.
//
// Two regimes.  LIST rounds (more than 64 active rows: the first few hundred rounds): the active rows are a list in
// global memory, a wave takes four of them at a time (row ids, then the four caches, requested together); the bids of a
// round meet in the per-column 64-bit atomic-min words `bid`.  CHAIN rounds (<= 64 active rows -- the long tail of the
// price wars, thousands of rounds): every wave holds up to four rows IN REGISTERS; the row a slot works on in the next round
// is the owner it displaces, known BEFORE the round's barrier, so that row's cache is requested at once and has arrived when
// the next round starts; bids meet in LDS (a ballot finds a better bid on the same column), two barriers per round and no
// global round trip on the path.  When half of the rows have dropped out the rest is dealt out again, one round-robin over
// the waves.  Both regimes realise the same round (a pure function of the state).
// ------------------------------------------------------------------------------------------------------------------
constexpr int ACS = 4;                 // rows per wave in a chain round / requested together in a list round
constexpr int ASL = WNW * ACS;         // slots of a chain round

struct ArrShared {
    int cnt[2];
    int retired, dense, ndeal;
    int pause;                          // the list rounds return to the driver for fresh row caches
    int wcnt[WNW];
    int sm_j[ASL], sm_i[ASL];
    float sm_p[ASL];
    int deal[ASL];
    int rf_cnt[WNW];                    // cache refresh (a wave rebuilds the cache of the row it just read in full): staging
    uint32_t rf_col[WNW][KC];
    float rf_val[WNW][KC];
};

constexpr size_t ARR_SHARED_BYTES = (sizeof(ArrShared) + 15) / 16 * 16;     // (in the dynamic region: a kernel's static LDS is limited to 2 KB here)
size_t wide_arr_lds_bytes(int n, bool vlds, bool clds) {
    const size_t npad = ((size_t)n + 3) & ~(size_t)3;
    return ARR_SHARED_BYTES + ((npad * ((vlds ? 4 : 0) + (clds ? 2 : 0)) + 15) / 16) * 16;
}
bool wide_arr_vlds(int n) { return n <= 65534 && wide_arr_lds_bytes(n, true, true) + 1024 <= (size_t)LDS_DYNAMIC_MAX; }
bool wide_arr_clds(int n) { return n <= 65534 && wide_arr_lds_bytes(n, false, true) + 1024 <= (size_t)LDS_DYNAMIC_MAX; }

template <bool VLDS, bool CLDS> struct ArrCtx {
    WideArgs a;
    float *s_v; uint16_t *s_cs; ArrShared *s;
    int lane;
    __device__ __forceinline__ float getv(int j) const { return VLDS ? s_v[j] : ld_sc1(a.v + j); }
    __device__ __forceinline__ int getcs(int j) const {
        if (CLDS) { const uint16_t x = s_cs[j]; return x == 0xFFFFu ? -1 : (int)x; }
        return ld_sc1(a.colsol + j);
    }
    // a won bid: price, owner, displaced owner change together (LDS copies and global)
    __device__ __forceinline__ void apply(int i, int jt, float pt, float ct, int i0) const {
        if (VLDS) s_v[jt] = pt;
        if (CLDS) s_cs[jt] = (uint16_t)i;
        a.v[jt] = pt; a.colsol[jt] = i; a.rowsol[i] = jt; a.cassign[jt] = ct;
        if (i0 >= 0) a.rowsol[i0] = -1;
    }
    // exact lexicographic top-2 of the whole row (the cache could not certify) -- and a fresh cache for the row against the
    // current prices, so that its next bids are certified again (in a price war the same few rows bid thousands of times).
    // The new floor is one of the 64 per-lane minima of the sweep (sorted; the 35th, else the 17th, 8th ... smallest: SC_FLOOR_POS): every
    // column below it is collected in a second sweep of the now L2-resident row; more than 63 of them -> the next candidate.
    // (Inlined on purpose: as an out-of-line call its results travel through scratch memory, and every bid -- also the
    // certified ones -- then stores and reloads them through the vector memory path.)
    __device__ __forceinline__ void top2_full(int i, int w, uint32_t &col, float &val, float &u1, int &j1, float &c1, float &vj1,
                                              float &u2, int &j2, float &c2, float &vj2) const {
        const int n = a.n;
        const float *__restrict__ row = a.cost + wrow_off(a.rowmap, i, a.ld);
        K2 d; d.m1 = KEYMAX; d.m2 = KEYMAX;
        wave_row_sweep(row, n, lane, [&](int c, float x) { k2_push(d, mkkey(x - getv(c), (uint32_t)c)); });
        uint32_t lm = (uint32_t)(d.m1 >> 32);                     // this lane's smallest reduced cost (ordered)
        d = k2_wave_allreduce(d);
        u1 = key_val(d.m1); j1 = (int)(uint32_t)d.m1; c1 = uni(row[j1]); vj1 = uni(getv(j1));
        u2 = INFINITY; j2 = -1; c2 = 0.0f; vj2 = 0.0f;
        if (d.m2 != KEYMAX) { u2 = key_val(d.m2); j2 = (int)(uint32_t)d.m2; c2 = uni(row[j2]); vj2 = uni(getv(j2)); }
        if (lane == 0) atomicAdd(&s->dense, 1);
        // ---- the row's new cache ----
#pragma unroll
        for (int k = 2; k <= 64; k <<= 1) {                       // bitonic sort of the 64 lane minima, ascending over the lanes
#pragma unroll
            for (int j = k >> 1; j > 0; j >>= 1) {
                const uint32_t o = (uint32_t)__shfl_xor((int)lm, j);
                const bool take_min = ((lane & j) == 0) == ((lane & k) == 0);
                lm = take_min ? umin32(lm, o) : (lm > o ? lm : o);
            }
        }
        uint32_t tk = 0;                                           // ordered floor; 0 = none found
        int cnt = 0;
        for (int pos = SC_FLOOR_POS; pos >= 2 && !tk; pos = (pos + 1) / 2 - 1) {
            const uint32_t cand = rdlane(lm, pos);
            if (cand == 0xFFFFFFFFu) continue;
            if (lane == 0) s->rf_cnt[w] = 0;
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            wave_row_sweep(row, n, lane, [&](int c, float x) {
                if (f2ord(x - getv(c)) < cand) {
                    const int p = atomicAdd(&s->rf_cnt[w], 1);
                    if (p < KCU) { s->rf_col[w][p] = (uint32_t)c; s->rf_val[w][p] = x; }
                }
            });
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            cnt = uni(s->rf_cnt[w]);
            if (cnt <= KCU) tk = cand;
        }
        const float tau = tk ? ord2f(tk) : -INFINITY;
        uint32_t kc = (tk && lane < cnt) ? s->rf_col[w][lane] : COLSENT;
        float kv = (tk && lane < cnt) ? s->rf_val[w][lane] : 0.0f;
#pragma unroll
        for (int k = 2; k <= 64; k <<= 1) {                       // cache rows are kept sorted by column (unused slots last)
#pragma unroll
            for (int j = k >> 1; j > 0; j >>= 1) {
                const uint32_t pk = (uint32_t)__shfl_xor((int)kc, j);
                const float pv = __shfl_xor(kv, j);
                const bool take_min = ((lane & j) == 0) == ((lane & k) == 0);
                const bool sw = take_min ? (pk < kc) : (pk > kc);
                kc = sw ? pk : kc; kv = sw ? pv : kv;
            }
        }
        if (lane == KCU) { kc = COLSENT; kv = tau; }               // (at most 63 entries: lane 63 held a sentinel)
        a.cache_col[(int64_t)i * KC + lane] = kc;
        a.cache_val[(int64_t)i * KC + lane] = kv;
        col = kc; val = kv;
    }
    // the bid of row i (its cache row in col / val, lane = entry): target column jt (-1: the row retires), price, raw cost of
    // the entry, and the owner it would displace
    // eps > 0 (a scaled phase): every bid lowers its column's price by the gap + eps, by one ulp at least -- no claims, nobody retires
    __device__ __forceinline__ void bid_of(int i, int w, uint32_t &col, float &val, int &jt, float &pt, float &ct, int &i0, float eps = 0.0f) const {
        // cache rows are sorted by column: among equal reduced costs the lowest lane is the lowest column, so the
        // lexicographic (value, column) top-2 is two 32-bit min reductions and two ballots
        const float tau = rdlane(val, KCU);
        const bool valid = lane < KCU && col != COLSENT;
        const float vj = valid ? getv((int)col) : 0.0f;
        const uint32_t key = valid ? f2ord(val - vj) : 0xFFFFFFFFu;
        const uint32_t k1 = wave_min_u32(key);
        const int l1 = __ffsll((unsigned long long)__ballot(key == k1)) - 1;
        const uint32_t key2 = lane == l1 ? 0xFFFFFFFFu : key;
        const uint32_t k2 = wave_min_u32(key2);
        float u1, u2, c1, c2, vj1, vj2;
        int j1, j2;
        if (k2 != 0xFFFFFFFFu && ord2f(k2) < tau) {           // the cached top-2 IS the row's lexicographic top-2
            const int l2 = __ffsll((unsigned long long)__ballot(key2 == k2)) - 1;
            u1 = ord2f(k1); j1 = (int)rdlane(col, l1); c1 = rdlane(val, l1); vj1 = rdlane(vj, l1);
            u2 = ord2f(k2); j2 = (int)rdlane(col, l2); c2 = rdlane(val, l2); vj2 = rdlane(vj, l2);
        } else {
            top2_full(i, w, col, val, u1, j1, c1, vj1, u2, j2, c2, vj2);
        }
        jt = -1; pt = 0.0f; ct = 0.0f; i0 = -1;
        const int o1 = uni(getcs(j1));
        if (eps > 0.0f) {
            float p = vj1 - ((u2 - u1) + eps);
            if (!(p < vj1)) p = pred_f32(vj1);
            jt = j1; pt = p; ct = c1; i0 = o1;
            jt = uni(jt); pt = uni(pt); ct = uni(ct); i0 = uni(i0);
            return;
        }
        const float p = vj1 - (u2 - u1);
        if (p < vj1) { jt = j1; pt = p; ct = c1; i0 = o1; }
        else if (o1 < 0) { jt = j1; pt = vj1; ct = c1; }
        else if (j2 >= 0 && u2 == u1 && uni(getcs(j2)) < 0) { jt = j2; pt = vj2; ct = c2; }
        jt = uni(jt); pt = uni(pt); ct = uni(ct); i0 = uni(i0);
    }
};

// The rounds on the whole chip: the phase machine of the row reduction (oracle/jv_oracle_impl.h, WIDE MODE).
//   LEGACY   eps = 0 rounds from the column reduction's state (claims, retirements).  After SC_K0 of them an instance whose active
//            list is still longer than wide_stop(n) -- generic costs: no ties to retire on, price wars without end -- SCALES; any
//            other one goes on until its list is short (<= 64 rows: the chain rounds of wide_arr take over) or empty.
//   EPS      phase k: every row unassigned, prices kept; rounds with eps_k = eps_0 / 2^k (every bid lowers its column's price by the
//            gap + eps_k) until the list is down to wide_stop(n) rows -- the sequential tail of a phase is cut, the next phase
//            takes every row up again.  eps_0 = 2^SC_EMULT x the median binade of the rows' gaps at the post-column-reduction prices.
//   FINAL    the same with eps = 0 and the claim / retire rules: what it leaves free goes to the searches.
// A round is ONE launch over all CUs (wide_sc_round).  Launch L does, a wave per row that bid in launch L - 1: the RESOLUTION of that
// row's bid -- did it win its column (the column's bid word)?  then price, owner, displaced owner are written to the arrays -- and at
// once the BID of the row that takes its place in the next round (the row itself if it lost, the owner it displaced if it won): no
// list is built in between, the wave that knows the outcome makes the next bid.  So the arrays (v, colsol) run ONE ROUND LATE while a
// launch is under way -- a column that received a bid in launch L - 1 has its new price and owner in its bid word (the winner's), and
// that is where the bids of launch L read them (word of launch L - 1 -> fresh; else the arrays, complete through launch L - 2);
// bid words are double-buffered by the launch's parity (launch L reads buffer (L - 1) & 1 and merges into buffer L & 1).  Full-row
// bids read the arrays and, through a bitmap of the columns bid for in launch L - 1 (three bitmaps in rotation), the fresh words.
// The bids of launch L are SPECULATIVE: whether the round they belong to takes place at all (or the phase ended with the list
// launch L - 1 left: its length is known only when that launch is over) is what launch L + 1 decides, from the same pure function of
// (state, list length) as the oracle -- if not, the bids are dropped: a bid changes nothing but bid words, records and counters kept
// per launch.  A phase boundary is a launch too: everything unassigned, and every row bids (nothing to resolve, no owners).
// The driver enqueues launches in groups and learns after each group who is through, one group late (the next group is queued
// before it asks: the chip never waits for the host; launches of a machine that is through return at once).
// The bid word of a column: | 12 bits ~(launch - base) | 32 bits ordered price | 20 bits row |, merged with an atomic min: within a
// launch the lowest (price, row) wins, and ANY bid of a later launch beats what earlier ones left behind -- the words are never reset
// between rounds; wide_sc_wipe (every 2048 launches per buffer) resets them and moves the buffer's `base`.
// ---- the machine's bids.  A row whose cache certifies its top-2 is one wave's work (the chain of a bid is L2 round trips: what
// counts is how many bids are in flight, so a wave per bid while the chip has room).  A row whose cache cannot certify is read in
// full -- by the WHOLE workgroup, after the wave's certified bids of the iteration: one wave sweeping an 80 KB row three times
// (wide_arr's top2_full) is 170 us, and the round waits for its slowest bid.  Prices and owners do not change while the bids of
// a round are made (the resolution is the next launch): plain loads, 16 bytes of the row and of the prices per lane and step.
struct ScShared {
    int nq, cnt, fill_, obase;
    uint32_t cand;
    int lrow[HEADB];                   // rows that bid out of the tile being resolved
    int qrow[HEADB / 64], qslot[HEADB / 64];
    unsigned long long km1[HEADB / 64], km2[HEADB / 64];
    uint32_t lmin[HEADB];
    uint32_t ccol[KC];
    float cval[KC];
};
constexpr size_t SC_SHARED_BYTES = (sizeof(ScShared) + 15) / 16 * 16;

// Where a launch's bids read prices and owners: the bid words of the launch before (fresh: that column's winner) or the arrays.
struct ScView {
    const unsigned long long *wsrc;   // bid words of launch L - 1 (null: none -- the first launch, a phase boundary)
    const uint32_t *pr;               // the prices as of the end of launch L - 1 (ordered; the machine's own price arrays); null: a.v holds them
    uint32_t tg;                      // tag of launch L - 1 in those words
    bool own_none;                    // a phase boundary: every column is unassigned (the arrays are being cleared by this very launch)
};
__device__ __forceinline__ bool sc_word_fresh(const ScView &vw, unsigned long long w) {
    return (uint32_t)(w >> 52) == vw.tg && ((uint32_t)w & 0xFFFFFu) != 0xFFFFFu;
}
__device__ __forceinline__ float sc_word_price(unsigned long long w) { return ord2f((uint32_t)(w >> 20)); }
// price and owner of column c as of the end of launch L - 1 (a dependent word load only where there is a word to ask)
__device__ __forceinline__ void sc_price_owner(const WideArgs &a, const ScView &vw, int c, float &p, int &o) {
    p = vw.pr ? ord2f(vw.pr[c]) : a.v[c]; o = vw.own_none ? -1 : a.colsol[c];
    if (vw.wsrc) { const unsigned long long w = vw.wsrc[c]; if (sc_word_fresh(vw, w)) o = (int)((uint32_t)w & 0xFFFFFu); }
}

// the decision of a bid from its row's lexicographic top-2 (oracle: JV_WIDE_ROUND): target column (-1: the row retires), price, raw cost
// of the entry, the owner it would displace (o1 / o2: the owners of the two columns).  eps > 0 (a scaled phase): every bid lowers its
// column's price by the gap + eps, by one ulp at least -- no claims, nobody retires
struct Top2 { float u1, c1, vj1, u2, c2, vj2; int j1, j2, o1, o2; };
__device__ __forceinline__ void sc_decide(const Top2 &t, float eps, int &jt, float &pt, float &ct, int &i0) {
    jt = -1; pt = 0.0f; ct = 0.0f; i0 = -1;
    const int o1 = t.o1;
    if (eps > 0.0f) {
        float p = t.vj1 - ((t.u2 - t.u1) + eps);
        if (!(p < t.vj1)) p = pred_f32(t.vj1);
        jt = t.j1; pt = p; ct = t.c1; i0 = o1;
    } else {
        const float p = t.vj1 - (t.u2 - t.u1);
        if (p < t.vj1) { jt = t.j1; pt = p; ct = t.c1; i0 = o1; }
        else if (o1 < 0) { jt = t.j1; pt = t.vj1; ct = t.c1; }
        else if (t.j2 >= 0 && t.u2 == t.u1 && t.o2 < 0) { jt = t.j2; pt = t.vj2; ct = t.c2; }
    }
    jt = uni(jt); pt = uni(pt); ct = uni(ct); i0 = uni(i0);
}
// one wave: the top-2 from the row's cache (lane = entry); false: the cache cannot certify it.  The prices of the 63 cached columns
// are gathered from the machine's price array (complete through the launch before); the owners of the two columns that matter are
// read last -- a column's bid word of the launch before if it is fresh (its winner), else the owner array.
// GOWN: words and owners of all cached columns are gathered with the prices (a launch with few bids is a chain of round trips: one less;
// for a launch with many bids that tripled the lines a bid pulls in: 8 000 bids took 60 us)
template <bool GOWN = false>
__device__ __forceinline__ bool sc_top2_cached(const WideArgs &a, const ScView &vw, int lane, uint32_t col, float val, Top2 &t) {
    const float tau = rdlane(val, KCU);
    const bool valid = lane < KCU && col != COLSENT;
    const float vj = valid ? (vw.pr ? ord2f(vw.pr[col]) : a.v[col]) : 0.0f;
    int ow = -1;
    if (GOWN && !vw.own_none) {
        ow = valid ? a.colsol[col] : -1;
        if (vw.wsrc) { const unsigned long long w = valid ? vw.wsrc[col] : ~0ull; if (sc_word_fresh(vw, w)) ow = (int)((uint32_t)w & 0xFFFFFu); }
    }
    const uint32_t key = valid ? f2ord(val - vj) : 0xFFFFFFFFu;
    const uint32_t k1 = wave_min_u32(key);
    const int l1 = __ffsll((unsigned long long)__ballot(key == k1)) - 1;
    const uint32_t key2 = lane == l1 ? 0xFFFFFFFFu : key;
    const uint32_t k2 = wave_min_u32(key2);
    if (!(k2 != 0xFFFFFFFFu && ord2f(k2) < tau)) return false;
    const int l2 = __ffsll((unsigned long long)__ballot(key2 == k2)) - 1;
    t.u1 = ord2f(k1); t.j1 = (int)rdlane(col, l1); t.c1 = rdlane(val, l1); t.vj1 = rdlane(vj, l1); t.o1 = (int)rdlane((uint32_t)ow, l1);
    t.u2 = ord2f(k2); t.j2 = (int)rdlane(col, l2); t.c2 = rdlane(val, l2); t.vj2 = rdlane(vj, l2); t.o2 = (int)rdlane((uint32_t)ow, l2);
    if (vw.own_none) { t.o1 = -1; t.o2 = -1; }
    else if (!GOWN) {
        const int c1 = a.colsol[t.j1], c2 = a.colsol[t.j2];        // (all four requested together)
        unsigned long long w1 = ~0ull, w2 = ~0ull;
        if (vw.wsrc) { w1 = vw.wsrc[t.j1]; w2 = vw.wsrc[t.j2]; }
        t.o1 = sc_word_fresh(vw, uni(w1)) ? (int)((uint32_t)uni(w1) & 0xFFFFFu) : uni(c1);
        t.o2 = sc_word_fresh(vw, uni(w2)) ? (int)((uint32_t)uni(w2) & 0xFFFFFu) : uni(c2);
    }
    return true;
}
// the whole workgroup (HEADB threads): f(column, cost, price) for every column of the row, 16 bytes of row and prices per lane and step
// (the prices: the machine's ordered price array, or a.v at a phase boundary)
template <int U, typename F> __device__ __forceinline__ void block_row_sweep(const float *__restrict__ row, const float *__restrict__ v, const ScView &vw, int n, F &&f) {
    const int nq = (n + 3) >> 2;
    const float4 *__restrict__ r4 = reinterpret_cast<const float4 *>(row);
    const float4 *__restrict__ v4 = reinterpret_cast<const float4 *>(vw.pr ? reinterpret_cast<const float *>(vw.pr) : v);   // (16-byte aligned, whole quads stay in range)
    const bool ordered = vw.pr != nullptr;
    for (int q0 = threadIdx.x; q0 < nq; q0 += HEADB * U) {
        float4 x[U], p[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int q = q0 + HEADB * u;
            x[u] = q < nq ? r4[q] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            p[u] = q < nq ? v4[q] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int q = q0 + HEADB * u, c = q * 4;
            if (q >= nq) continue;
            if (ordered) { p[u].x = ord2f(__float_as_uint(p[u].x)); p[u].y = ord2f(__float_as_uint(p[u].y)); p[u].z = ord2f(__float_as_uint(p[u].z)); p[u].w = ord2f(__float_as_uint(p[u].w)); }
            f(c, x[u].x, p[u].x);
            if (c + 1 < n) f(c + 1, x[u].y, p[u].y);
            if (c + 2 < n) f(c + 2, x[u].z, p[u].z);
            if (c + 3 < n) f(c + 3, x[u].w, p[u].w);
        }
    }
}
// the whole workgroup: exact lexicographic top-2 of row i -- and a fresh cache for it against the current prices (floor = one of the 64
// minima of the columns c with (c / 4) % 64 == l, sorted: the 35th, else the 17th, 8th ... smallest; the columns below it are collected in
// a second sweep of the now L2-resident row; more than 63 of them -> the next candidate).  Every thread returns the same Top2.
template <int U>
__device__ __forceinline__ Top2 sc_top2_block(const WideArgs &a, const ScView &vw, ScShared &ss, int i, bool rebuild) {
    const int n = a.n, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const float *__restrict__ row = a.cost + wrow_off(a.rowmap, i, a.ld);
    K2 d; d.m1 = KEYMAX; d.m2 = KEYMAX;
    block_row_sweep<U>(row, a.v, vw, n, [&](int c, float x, float vc) { k2_push(d, mkkey(x - vc, (uint32_t)c)); });
    const uint32_t my_min = (uint32_t)(d.m1 >> 32);              // the smallest reduced cost among THIS thread's columns (ordered)
    ss.lmin[tid] = my_min;
    d = k2_wave_allreduce(d);
    if (lane == 0) { ss.km1[w] = d.m1; ss.km2[w] = d.m2; }
    __syncthreads();
    K2 g; g.m1 = ss.km1[0]; g.m2 = ss.km2[0];
#pragma unroll
    for (int k = 1; k < HEADB / 64; k++) { K2 o; o.m1 = ss.km1[k]; o.m2 = ss.km2[k]; k2_merge(g, o); }
    Top2 t;
    t.u1 = key_val(g.m1); t.j1 = (int)(uint32_t)g.m1; t.c1 = row[t.j1]; sc_price_owner(a, vw, t.j1, t.vj1, t.o1);
    t.u2 = INFINITY; t.j2 = -1; t.c2 = 0.0f; t.vj2 = 0.0f; t.o2 = -1;
    if (g.m2 != KEYMAX) { t.u2 = key_val(g.m2); t.j2 = (int)(uint32_t)g.m2; t.c2 = row[t.j2]; sc_price_owner(a, vw, t.j2, t.vj2, t.o2); }
    if (!rebuild) { __syncthreads(); return t; }                   // (the staging words are free again for the next row)
    // ---- the row's new cache ----
    uint32_t lm = 0xFFFFFFFFu;
    if (w == 0) {
#pragma unroll
        for (int k = 0; k < HEADB / 64; k++) lm = umin32(lm, ss.lmin[k * 64 + lane]);
#pragma unroll
        for (int k = 2; k <= 64; k <<= 1) {                       // bitonic sort of the 64 minima, ascending over the lanes
#pragma unroll
            for (int j = k >> 1; j > 0; j >>= 1) {
                const uint32_t o = (uint32_t)__shfl_xor((int)lm, j);
                const bool take_min = ((lane & j) == 0) == ((lane & k) == 0);
                lm = take_min ? umin32(lm, o) : (lm > o ? lm : o);
            }
        }
    }
    uint32_t tk = 0;                                               // ordered floor; 0 = none found
    int cnt = 0;
    for (int pos = SC_FLOOR_POS; pos >= 2 && !tk; pos = (pos + 1) / 2 - 1) {
        if (w == 0 && lane == 0) { ss.cand = rdlane(lm, pos); ss.cnt = 0; }
        __syncthreads();
        const uint32_t cand = ss.cand;
        if (cand != 0xFFFFFFFFu && my_min < cand)                    // (a thread none of whose columns lies below the candidate reads nothing: ~4 of 5)
            block_row_sweep<U>(row, a.v, vw, n, [&](int c, float x, float vc) {
                if (f2ord(x - vc) < cand) {
                    const int p = atomicAdd(&ss.cnt, 1);
                    if (p < KCU) { ss.ccol[p] = (uint32_t)c; ss.cval[p] = x; }
                }
            });
        __syncthreads();
        cnt = ss.cnt;
        if (cand != 0xFFFFFFFFu && cnt <= KCU) tk = cand;
        __syncthreads();                                           // (everybody has read the count before the next candidate resets it)
    }
    if (w == 0) {
        const float tau = tk ? ord2f(tk) : -INFINITY;
        uint32_t kc = (tk && lane < cnt) ? ss.ccol[lane] : COLSENT;
        float kv = (tk && lane < cnt) ? ss.cval[lane] : 0.0f;
#pragma unroll
        for (int k = 2; k <= 64; k <<= 1) {                       // cache rows are kept sorted by column (unused slots last)
#pragma unroll
            for (int j = k >> 1; j > 0; j >>= 1) {
                const uint32_t pk = (uint32_t)__shfl_xor((int)kc, j);
                const float pv = __shfl_xor(kv, j);
                const bool take_min = ((lane & j) == 0) == ((lane & k) == 0);
                const bool sw = take_min ? (pk < kc) : (pk > kc);
                kc = sw ? pk : kc; kv = sw ? pv : kv;
            }
        }
        if (lane == KCU) { kc = COLSENT; kv = tau; }               // (at most 63 entries: lane 63 held a sentinel)
        a.cache_col[(int64_t)i * KC + lane] = kc;
        a.cache_val[(int64_t)i * KC + lane] = kv;
    }
    return t;
}

__device__ __forceinline__ unsigned long long bidkey(long long round, float price, int row) {
    return ((unsigned long long)(~(uint32_t)round & 0xFFFu) << 52) | ((unsigned long long)f2ord(price) << 20) | (uint32_t)row;
}
__device__ __forceinline__ bool bid_won(unsigned long long word, int row) { return (int)((uint32_t)word & 0xFFFFFu) == row; }

struct ArrHead { int cnt[2]; int started, free_cr; long long round, bids; int retired, dense; int done, launches; long long list_rounds; int no_more, pad_; };
static_assert(sizeof(ArrHead) <= sizeof(LapStatus::arr), "ArrHead lives in LapStatus::arr");
__device__ __forceinline__ ArrHead *arr_head(const WideArgs &a) { return reinterpret_cast<ArrHead *>(lap_status(a.misc)->arr); }

// ---- the machine's memory beyond the driver's arrays (WideArgs.scx, wide_sc_ext_bytes(n) bytes, 256-byte aligned): the two buffers of
// bid words (all-ones at the start: the first wide_sc_ones_bytes(n) bytes), the machine's two price arrays (ordered floats; wide_sc_init
// copies the prices in), the bid records of a launch (two buffers by the launch's parity: 16 bytes { row, column or -1, price,
// owner it would displace } and the raw cost of the entry).
struct ScRec { int i, jt; float pt; int i0; };
// (accessors instead of a table of pointers: a table indexed by the launch's parity would live in scratch memory)
__device__ __forceinline__ unsigned long long *sc_words(char *scx, int n, int b) { return reinterpret_cast<unsigned long long *>(scx + scx_off_words(n, b)); }
__device__ __forceinline__ uint32_t *sc_price(char *scx, int n, int k) { return reinterpret_cast<uint32_t *>(scx + scx_off_price(n, k)); }
__device__ __forceinline__ ScRec *sc_recs(char *scx, int n, int b) { return reinterpret_cast<ScRec *>(scx + scx_off_recs(n, b)); }
__device__ __forceinline__ float *sc_rcts(char *scx, int n, int b) { return reinterpret_cast<float *>(scx + scx_off_rcts(n, b)); }

__device__ __forceinline__ float sc_eps_of(const ScCtl *sc, int k) {       // eps of phase k, 0 = there is no such phase
    if (k >= SC_NPH) return 0.0f;
    const int ek = sc->e0 - SC_ESTEP * k;
    if (ek < 1) return 0.0f;
    const float eps = __uint_as_float((uint32_t)ek << 23);
    return eps < sc->epsmin ? 0.0f : eps;
}
// the step the machine takes from state S with `na` active rows (oracle: the head of the phase machine's loop; every thread of a
// launch computes the same)
__device__ __forceinline__ ScSlot sc_step(const ScCtl *sc, const ScSlot &S, int na, int n, long long max_rounds) {
    ScSlot N = S;
    N.act = SC_ACT_NONE; N.fresh = 0;
    if (S.mode >= SC_HANDOVER) return N;
    // (the budget of rounds ends the LEGACY rounds and the scaled phases, never the FINAL phase: the assignments a scaled phase leaves
    //  satisfy eps-complementary slackness only, the searches need the eps = 0 phase's)
    const bool over = S.total >= max_rounds;
    bool next_phase = false, last = false;
    if (S.mode == SC_LEGACY) {
        if (over || na == 0) { N.mode = SC_DONE; return N; }
        if (S.rip == SC_K0 && na > sc->stop && sc->e0 > 0) { next_phase = true; N.k = -1; }
        else if (S.rip >= SC_K0 && na <= ASL) { N.mode = SC_HANDOVER; return N; }
    } else if (S.mode == SC_EPS) {
        if (over) { next_phase = true; last = true; }
        else if (S.rip >= 1 && (na <= sc->stop || S.rip >= SC_PHCAP)) next_phase = true;
    } else if (S.rip >= 1 && (na <= (sc->stop < SC_STOP_FINAL ? sc->stop : SC_STOP_FINAL) || S.rip >= SC_PHCAP)) { N.mode = SC_DONE; return N; }
    if (next_phase) {
        N.k = N.k + 1;
        const float eps = last ? 0.0f : sc_eps_of(sc, N.k);
        N.mode = eps > 0.0f ? SC_EPS : SC_FINAL; N.eps = eps; N.rip = 0; N.act = SC_ACT_RESET;
        return N;
    }
    N.act = SC_ACT_ROUND; N.rip = S.rip + 1; N.total = S.total + 1; N.bids = S.bids + na;
    return N;
}

__global__ __launch_bounds__(HEADB) void wide_sc_init(const WideArgs *__restrict__ batch) {
    const WideArgs a = load_wide_args(batch, blockIdx.y);
    ScCtl *sc = reinterpret_cast<ScCtl *>(a.sc);
    const int n = a.n, lane = threadIdx.x & 63;
    for (int i0 = blockIdx.x * HEADB; i0 < n; i0 += gridDim.x * HEADB) {
        const int i = i0 + threadIdx.x;
        const bool fr = i < n && a.rowsol[i] < 0;
        const uint64_t m = __ballot(fr);
        int base = 0;
        if (lane == 0 && m) base = atomicAdd(&sc->rnd[2].cnt, __popcll(m));        // (the list launch 0 reads: cell (0 - 1) mod 3)
        base = __shfl(base, 0);
        if (fr) a.act0[base + __popcll(m & lanemask_lt())] = i;
        if (i < n) { const uint32_t o = f2ord(a.v[i]); sc_price((char *)a.scx, n, 0)[i] = o; sc_price((char *)a.scx, n, 1)[i] = o; }     // the machine's price arrays
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        // the median binade of the gaps (wide_rt's histogram), eps_0 = 2^SC_EMULT times it; no scaling when half the gaps are zero
        long long cum = 0; int me = 0;
        for (int e = 0; e < 256; e++) { cum += sc->hist[e]; if (cum * 2 >= n) { me = e; break; } }
        sc->e0 = me > 0 ? (me + SC_EMULT > 254 ? 254 : me + SC_EMULT) : 0;
        sc->epsmin = __uint_as_float(sc->vmaxbits) * 1.1920928955078125e-07f;
        sc->stop = wide_stop(n);
        ScSlot S; S.mode = SC_LEGACY; S.k = 0; S.rip = 0; S.fresh = 1; S.act = SC_ACT_NONE; S.eps = 0.0f; S.total = 0; S.bids = 0; S.heavy = 0; S.pad_ = 0;
        sc->slot[0] = S;
    }
}

// Launch L of the machine (see the header above): the step the state and the length of the list that bid in launch L - 1 ask for --
//   ROUND  those bids stand: a wave per bid resolves it and bids at once for the row that takes its place;
//   RESET  a phase begins (those bids are dropped): everything unassigned, every row bids;
//   none   the machine is through (those bids are dropped; their rows are the list it leaves) --
// or, in launch 0, the first bids of the rows the column reduction left free.
template <int U, bool DIRECT>
__global__ __launch_bounds__(HEADB) void wide_sc_round(const WideArgs *__restrict__ batch, int L, int n_arg, char *sc_direct, char *scx_direct, int *hs, int small_max) {
    extern __shared__ __align__(16) unsigned char w_smem[];
    // DIRECT (one problem): the control block, the machine's arrays and n are kernel arguments, so the state and -- unconditionally, a
    // wave per slot -- the record a launch with few bids will resolve are requested before the argument block has arrived
    const WideArgs a = load_wide_args(batch, blockIdx.y);
    const int n = DIRECT ? n_arg : a.n;
    ScCtl *sc = reinterpret_cast<ScCtl *>(DIRECT ? sc_direct : (char *)a.sc);
    char *scx = DIRECT ? scx_direct : (char *)a.scx;
    const int lane = threadIdx.x & 63, w = uni((int)(threadIdx.x >> 6));
    const int pb = (L + 1) & 1, cb = L & 1;                      // record / word buffers: the launch before, this launch
    const int rp = (L + 2) % 3, rc = L % 3, rn = (L + 1) % 3;    // per-launch cells and bitmaps: the launch before, this one, the next
    const ScRec *rsrc = sc_recs(scx, n, pb);
    const float *csrc = sc_rcts(scx, n, pb);
    const int slot_s = (int)blockIdx.x * (HEADB / 64) + w;
    int4 rr_s = make_int4(-1, -1, 0, -1);
    float rct_s = 0.0f;
    if (slot_s < n) { rr_s = *reinterpret_cast<const int4 *>(rsrc + slot_s); rct_s = csrc[slot_s]; }
    const ScSlot S = sc->slot[L & 1];
    const bool lead = blockIdx.x == 0 && threadIdx.x == 0;
    // (what the driver watches, pinned host memory: the launch under way -- reported by the batch's first problem whatever its state)
    if (lead && hs && blockIdx.y == 0) __hip_atomic_store(hs, L + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (S.mode >= SC_HANDOVER) {                                 // through: the state stays (both slots)
        if (lead && sc->slot[(L + 1) & 1].mode != S.mode) { ScSlot N = S; N.act = SC_ACT_NONE; sc->slot[(L + 1) & 1] = N; }
        return;
    }
    const int np = sc->rnd[rp].cnt;                              // rows that bid in launch L - 1 (launch 0: rows on wide_sc_init's list)
    const bool first = S.fresh != 0;
    ScSlot N;
    if (first) { N = S; N.fresh = 0; N.act = SC_ACT_NONE; } else N = sc_step(sc, S, np, n, a.max_rounds);
    const int act = N.act;
    const bool through = !first && act == SC_ACT_NONE;
    if (lead) {
        // what the driver watches besides the launch under way (pinned host memory, no synchronisation): the machines that are through, and
        // per problem "rebuild my row caches" -- the full-row bids since the last rebuild have reached a.arr_waste
        // (measured on the few-cell-type 20 000^2 instance: a rebuild whenever a.arr_waste full-row bids have been made -- ~14
        //  rebuilds of 1 ms -- gives a 25 ms row reduction; rebuilding only from n / 2 full-row bids per group on and never in the
        //  coarse phases 34 ms: a round waits for the workgroup with the most full-row bids, so few of them already cost every round)
        if (hs) {
            if (through) __hip_atomic_fetch_add(hs + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            else if (a.aug_seg == 0 && L - sc->want_mark >= 64 && sc->dense - sc->dense_mark >= a.arr_waste) {      // (once per 64 launches at most)
                sc->dense_mark = sc->dense; sc->want_mark = L;
                __hip_atomic_store(hs + 4 + blockIdx.y, L + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
        N.heavy = (long long)sc->dense * 32 > N.bids ? 1 : 0;
        sc->slot[(L + 1) & 1] = N;
        sc->rnd[rn].cnt = 0; sc->rnd[rn].retired = 0;
        if (first) { sc->free_cr = np; sc->rnd[rc].cnt = np; }
        if (act == SC_ACT_ROUND) sc->retired += sc->rnd[rp].retired;   // the round took place: its retirements count
        if (act == SC_ACT_RESET) { sc->phases += 1; sc->rnd[rc].cnt = n; }
        if (through) { sc->fin_buf = pb; sc->fin_cnt = np; }
    }
    if (through) return;
    // The machine's two price arrays (ordered floats, merged with atomic mins: prices only fall): launch L reads P[(L - 1) & 1] -- complete
    // through round L - 1 -- and merges into P[L & 1] (complete through round L - 2 when the launch starts) the bids it resolves (round L - 1)
    // and the bids it makes: complete through round L when it ends.  Dropped bids (a phase ended) have spoilt the array they were merged
    // into, P[(L - 1) & 1] at the phase boundary L: that launch reads the price array proper (a.v: complete, the resolutions wrote it)
    // and copies it over the spoilt one.
    uint32_t *pw = sc_price(scx, n, cb);
    if (act == SC_ACT_RESET) {
        uint32_t *pfix = sc_price(scx, n, pb);
        for (int i = blockIdx.x * HEADB + threadIdx.x; i < n; i += gridDim.x * HEADB) { a.rowsol[i] = -1; a.colsol[i] = -1; pfix[i] = f2ord(a.v[i]); }
    }
    // few bids to resolve: a wave per bid (below); else tiles
    // (an instance that bids from full rows a lot -- S.heavy -- takes the tiles even for few bids when it has the chip to itself (a batch's
    //  problems have 64-256 workgroups each: measured slower there): ONE bid per workgroup while there are workgroups enough: a full-row bid is the whole workgroup's work, and the launch waits for the workgroup with the most of them)
    const bool small = act == SC_ACT_ROUND && !(S.heavy && HEAVY_SPREAD && gridDim.x >= 512) && np <= small_max && np <= (int)gridDim.x * (HEADB / 64);
    if (small && (int)blockIdx.x * (HEADB / 64) >= np) return;
    ScShared &ss = *reinterpret_cast<ScShared *>(w_smem);
    if (threadIdx.x == 0) { ss.nq = 0; ss.fill_ = 0; ss.cnt = 0; }
    __syncthreads();
    ScView vw;
    vw.wsrc = act == SC_ACT_ROUND ? sc_words(scx, n, pb) : nullptr;
    vw.pr = act == SC_ACT_RESET ? nullptr : sc_price(scx, n, pb);
    vw.tg = ~(uint32_t)((long long)(L - 1) - (long long)sc->wbase[pb]) & 0xFFFu;
    vw.own_none = act == SC_ACT_RESET;
    unsigned long long *wdst = sc_words(scx, n, cb);
    ScRec *rdst = sc_recs(scx, n, cb);
    float *cdst = sc_rcts(scx, n, cb);
    const long long tag = (long long)L - (long long)sc->wbase[cb];
    const float eps = N.eps;
    // a coarse phase (eps_k many times the span of a row's 63 cached columns) moves the prices past every cache within a bid or two:
    // there a full-row bid does not rebuild its row's cache (half its cost) -- the later phases do, and keep their caches
    const bool refresh = !(N.mode == SC_EPS && N.k < SC_COARSE);
    int retired = 0, dense = 0;                                   // (lane 0 of every wave)
    int *ocnt = &sc->rnd[rc].cnt;
    auto record = [&](int oslot, int i, const Top2 &t) {
        int jt, i0; float pt, ct;
        sc_decide(t, eps, jt, pt, ct, i0);
        if (lane == 0) {
            if (jt < 0) retired++;
            else {
                atomicMin(wdst + jt, bidkey(tag, pt, i));
                atomicMin(pw + jt, f2ord(pt));
            }
            *reinterpret_cast<int4 *>(rdst + oslot) = make_int4(i, jt, __float_as_int(pt), i0);
            cdst[oslot] = ct;
        }
    };
    // rows whose caches could not certify (queued in LDS): the whole workgroup reads each in full, one after the other
    auto full_rows = [&](int obase) {
        __syncthreads();
        const int nq = ss.nq;
        __syncthreads();
        if (nq) {
            if (threadIdx.x == 0) ss.nq = 0;
            for (int q = 0; q < nq; q++) {
                const int i = ss.qrow[q], oslot = obase + ss.qslot[q];
                const Top2 t = sc_top2_block<U>(a, vw, ss, i, refresh);
                if (w == 0) { record(oslot, i, t); dense++; }
            }
            __syncthreads();
        }
    };
    if (small) {
        // ---- a wave per bid of the launch before.  Everything the outcome decides between is requested with the word that decides
        // it: the caches of the row (it bids again if it lost) and of the owner it displaces (who bids if it won); the slot of the
        // new record comes from one atomic per workgroup that is in flight while the bid is made.
        const int ri = uni(rr_s.x), rj = uni(rr_s.y), r0 = uni(rr_s.w);
        int nxt = -1, rank = 0;
        uint32_t col = COLSENT; float val = 0.0f;
        if (slot_s < np && rj >= 0) {                               // (a retired row stays free and bids no more)
            if (lane == 0) atomicMin(pw + rj, f2ord(__int_as_float(rr_s.z)));     // (every bid of the round, won or lost: the lowest is the price)
            const unsigned long long word = vw.wsrc[rj];
            const uint32_t colA = a.cache_col[(int64_t)ri * KC + lane];
            const float valA = a.cache_val[(int64_t)ri * KC + lane];
            uint32_t colB = COLSENT; float valB = 0.0f;
            if (r0 >= 0) { colB = a.cache_col[(int64_t)r0 * KC + lane]; valB = a.cache_val[(int64_t)r0 * KC + lane]; }
            if (bid_won(uni(word), ri)) {
                if (lane == 0) {
                    a.v[rj] = __int_as_float(rr_s.z); a.colsol[rj] = ri; a.rowsol[ri] = rj; a.cassign[rj] = rct_s;
                    if (r0 >= 0) a.rowsol[r0] = -1;
                }
                nxt = r0; col = colB; val = valB;
            } else { nxt = ri; col = colA; val = valA; }
            if (nxt >= 0) { if (lane == 0) rank = atomicAdd(&ss.cnt, 1); rank = uni(rank); }
        }
        __syncthreads();
        int obase_r = 0;
        const int nl = ss.cnt;
        if (threadIdx.x == 0 && nl) obase_r = atomicAdd(ocnt, nl);
        Top2 t;
        bool have = false;
        if (nxt >= 0) {
            have = sc_top2_cached<true>(a, vw, lane, col, val, t);
            if (!have && lane == 0) { const int q = atomicAdd(&ss.nq, 1); ss.qrow[q] = nxt; ss.qslot[q] = rank; }
        }
        if (threadIdx.x == 0) ss.obase = obase_r;
        __syncthreads();
        const int obase = ss.obase;
        if (have) record(obase + rank, nxt, t);
        full_rows(obase);
    } else {
        // ---- every workgroup takes a contiguous run of the work (bids to resolve; rows at a phase boundary) in tiles of HEADB.
        // ROUND, per tile: first a THREAD per bid resolves it (record and word: coalesced / one gather; a winner's thread writes price,
        // owner, displaced owner) and the rows that bid next are gathered in LDS -- their records' slots come from ONE atomic on the
        // launch's counter per tile (a wave per bid with an atomic each: 20 000 atomics on one address made a phase's first launches
        // 130-170 us) -- then a WAVE per gathered row makes its bid.
        const int nwork = act == SC_ACT_RESET ? n : np;
        // (a run of at least 8 bids -- fewer atomics on the launch's counter -- unless the instance bids from full rows a lot: those a
        //  workgroup reads one after the other, and the launch waits for the workgroup with the most of them)
        const bool heavy = S.heavy != 0;
        const int chunk = std::max(act == SC_ACT_ROUND && !heavy ? 8 : (heavy && HEAVY_SPREAD && gridDim.x >= 512 && act == SC_ACT_ROUND ? 1 : HEADB / 64), (nwork + (int)gridDim.x - 1) / (int)gridDim.x);
        const int c_lo = std::min(nwork, (int)blockIdx.x * chunk), c_hi = std::min(nwork, c_lo + chunk);
        for (int t0 = c_lo; t0 < c_hi; t0 += HEADB) {
            const int tn = std::min(HEADB, c_hi - t0);           // work items of this tile
            int nlist = tn;                                       // rows that bid out of this tile
            if (act == SC_ACT_ROUND) {
                if (threadIdx.x == 0) ss.cnt = 0;
                __syncthreads();
                int nxt = -1;
                if ((int)threadIdx.x < tn) {
                    const int slot = t0 + (int)threadIdx.x;
                    const int4 rr = *reinterpret_cast<const int4 *>(rsrc + slot);
                    if (rr.y >= 0) {                                // (a retired row stays free and bids no more)
                        atomicMin(pw + rr.y, f2ord(__int_as_float(rr.z)));      // (every bid of the round, won or lost: the lowest is the price)
                        const unsigned long long word = vw.wsrc[rr.y];
                        const float rct = csrc[slot];
                        if (bid_won(word, rr.x)) {
                            a.v[rr.y] = __int_as_float(rr.z); a.colsol[rr.y] = rr.x; a.rowsol[rr.x] = rr.y; a.cassign[rr.y] = rct;
                            if (rr.w >= 0) a.rowsol[rr.w] = -1;
                            nxt = rr.w;                             // the displaced owner bids next (or nobody)
                        } else nxt = rr.x;
                    }
                }
                const uint64_t mb = __ballot(nxt >= 0);
                int wbase = 0;
                if (lane == 0 && mb) wbase = atomicAdd(&ss.cnt, __popcll(mb));
                wbase = __shfl(wbase, 0);
                const int lpos = wbase + __popcll(mb & lanemask_lt());
                if (nxt >= 0) ss.lrow[lpos] = nxt;
                __syncthreads();
                nlist = ss.cnt;
                if (threadIdx.x == 0 && nlist) ss.obase = atomicAdd(ocnt, nlist);
                __syncthreads();
            }
            const int obase = act == SC_ACT_ROUND ? ss.obase : t0;
            for (int e0 = 0; e0 < nlist; e0 += HEADB / 64) {     // (the same trips for every wave of the workgroup)
                const int e = e0 + w;
                if (e < nlist) {
                    const int i = act == SC_ACT_ROUND ? uni(ss.lrow[e]) : (act == SC_ACT_RESET ? t0 + e : uni(a.act0[t0 + e]));
                    const uint32_t col = a.cache_col[(int64_t)i * KC + lane];
                    const float val = a.cache_val[(int64_t)i * KC + lane];
                    Top2 t;
                    if (sc_top2_cached(a, vw, lane, col, val, t)) record(obase + e, i, t);
                    else if (lane == 0) { const int q = atomicAdd(&ss.nq, 1); ss.qrow[q] = i; ss.qslot[q] = e; }
                }
                full_rows(obase);
            }
        }
    }
    if (lane == 0) { if (retired) atomicAdd(&sc->rnd[rc].retired, retired); if (dense) atomicAdd(&sc->dense, dense); }
}

// before launch L: the bid words of ITS buffer start over (the other buffer holds the bids launch L resolves)
__global__ __launch_bounds__(HEADB) void wide_sc_wipe(const WideArgs *__restrict__ batch, int L) {
    const WideArgs a = load_wide_args(batch, blockIdx.y);
    ScCtl *sc = reinterpret_cast<ScCtl *>(a.sc);
    unsigned long long *wd = sc_words((char *)a.scx, a.n, L & 1);
    for (int j = blockIdx.x * HEADB + threadIdx.x; j < a.n; j += gridDim.x * HEADB) wd[j] = ~0ull;
    if (blockIdx.x == 0 && threadIdx.x == 0) sc->wbase[L & 1] = (unsigned long long)L;
}

// the machine is through (the next launch would be L): what wide_arr picks up -- the rows that were active when it stopped (for the
// chain rounds of a LEGACY problem: on the list its round's parity names), the counters; no_more: the rounds are over (budget, or a
// scaled problem's last phase)
__global__ void wide_sc_finish(const WideArgs *__restrict__ batch, int L) {
    const WideArgs a = load_wide_args(batch, blockIdx.x);
    ScCtl *sc = reinterpret_cast<ScCtl *>(a.sc);
    ArrHead *h = arr_head(a);
    const ScSlot S = sc->slot[L & 1];
    const int na = sc->fin_cnt, want = (int)(S.total & 1);
    const bool chain = S.mode == SC_HANDOVER;
    if (chain) {
        const ScRec *R = sc_recs((char *)a.scx, a.n, sc->fin_buf);
        int32_t *B = want ? a.act1 : a.act0;
        for (int q = threadIdx.x; q < na; q += blockDim.x) B[q] = R[q].i;
    }
    if (threadIdx.x == 0) {
        h->cnt[want] = na; h->cnt[want ^ 1] = 0; h->started = 1; h->free_cr = sc->free_cr; h->round = S.total; h->bids = S.bids;
        h->retired = sc->retired; h->dense = sc->dense; h->done = 0; h->launches = 0; h->list_rounds = S.total; h->no_more = chain ? 0 : 1;
        long long *tmr = lap_status(a.misc)->timers;
        tmr[WT_SCALED] = sc->phases > 0 ? 1 : 0; tmr[WT_PHASES] = sc->phases;
    }
}

template <bool VLDS, bool CLDS>
__global__ __launch_bounds__(WT) void wide_arr(const WideArgs *__restrict__ batch) {
    extern __shared__ __align__(16) unsigned char w_smem[];
    ArrShared &s = *reinterpret_cast<ArrShared *>(w_smem);
    ArrCtx<VLDS, CLDS> cx;
    cx.a = load_wide_args(batch, blockIdx.x);
    const WideArgs &a = cx.a;
    const int n = a.n, tid = threadIdx.x, lane = tid & 63, w = uni((int)(threadIdx.x >> 6));
    cx.s_v = reinterpret_cast<float *>(w_smem + ARR_SHARED_BYTES);
    cx.s_cs = reinterpret_cast<uint16_t *>(cx.s_v + (VLDS ? ((n + 3) & ~3) : 0));
    cx.s = &s; cx.lane = lane;
    const long long t_kernel0 = wall_clock64();
    // The rounds may take several launches (LapStatus::arr carries the state): like the searches of wide_aug, the
    // list rounds return to the driver when the row caches have gone stale -- a row whose cache cannot certify its bid reads its
    // full row and rebuilds its own cache, three sweeps on one wave; once those have cost what a rebuild of ALL caches by the
    // whole chip costs (a.arr_waste of them in this launch; or a.seg_quorum workgroups of the launch have asked), that is cheaper.
    ArrHead *h = arr_head(a);
    if (h->done) {                                               // finished in an earlier launch
        if (tid == 0 && a.seg_sync) a.seg_sync[1 + blockIdx.x] = a.seg_sync[1 + blockIdx.x] & 2;
        return;
    }
    if (tid == 0) { s.cnt[0] = 0; s.cnt[1] = 0; s.retired = 0; s.dense = 0; s.ndeal = 0; s.pause = 0; }
    if (CLDS)
        for (int j = tid; j < n; j += WT) {
            if (VLDS) cx.s_v[j] = a.v[j];
            const int o = a.colsol[j]; cx.s_cs[j] = o < 0 ? (uint16_t)0xFFFFu : (uint16_t)o;
        }
    __syncthreads();

    // the active list: what the phase machine on the whole chip left (wide_sc_finish), else every free row (in any order -- a
    // round does not depend on it)
    const bool headed = h->started != 0;
    int cur = 0;
    long long round = 0, bids = 0;
    if (headed) {
        round = h->round; bids = h->bids; cur = (int)(round & 1);
        if (tid == 0) { s.cnt[cur] = h->cnt[cur]; s.retired = h->retired; s.dense = h->dense; }
    } else {
        for (int i0 = 0; i0 < n; i0 += WT) {
            const int i = i0 + tid;
            const bool fr = i < n && a.rowsol[i] < 0;
            const uint64_t m = __ballot(fr);
            int base = 0;
            if (lane == 0 && m) base = atomicAdd(&s.cnt[0], __popcll(m));
            base = __shfl(base, 0);
            if (fr) a.act0[base + __popcll(m & lanemask_lt())] = i;
        }
    }
    __syncthreads();
    const int free_cr = headed ? h->free_cr : s.cnt[0];
    const long long t_start = wall_clock64();
    if (tid == 0) lap_status(a.misc)->timers[WT_ARR_SETUP_TICKS] = t_start - t_kernel0;
    long long t_list = 0, t_chain = 0, n_list = 0, n_chain = 0, n_deal = 0;
    int32_t *A = cur ? a.act1 : a.act0, *B = cur ? a.act0 : a.act1;
    int na = free_cr;
    const int dense0 = s.dense;
    const long long round0 = round;
    const bool no_more = h->no_more != 0;
    bool paused = false, announced = false;
    // ================= LIST rounds =================
    for (;;) {
        na = uni(s.cnt[cur]);
        if (na <= ASL || round >= a.max_rounds || no_more) break;
        if (uni(s.pause)) { paused = true; break; }
        if (round == round0 || (round & 0xFFF) == 0) {               // the bid words: wiped at the start and whenever their round tag wraps
            for (int j = tid; j < n; j += WT) a.bid[j] = ~0ull;
            __syncthreads();
        }
        for (int base = 0; base < na; base += ASL) {
            int ri[ACS]; uint32_t col[ACS]; float val[ACS];
#pragma unroll
            for (int q = 0; q < ACS; q++) { const int slot = base + q * WNW + w; ri[q] = slot < na ? uni(ld_sc1(A + slot)) : -1; }
#pragma unroll
            for (int q = 0; q < ACS; q++)
                if (ri[q] >= 0) { col[q] = a.cache_col[(int64_t)ri[q] * KC + lane]; val[q] = a.cache_val[(int64_t)ri[q] * KC + lane]; }
#pragma unroll
            for (int q = 0; q < ACS; q++) {
                if (ri[q] < 0) continue;
                const int slot = base + q * WNW + w;
                int jt, i0; float pt, ct;
                cx.bid_of(ri[q], w, col[q], val[q], jt, pt, ct, i0);
                if (lane == 0) {
                    if (jt < 0) atomicAdd(&s.retired, 1);
                    else atomicMin(a.bid + jt, bidkey(round, pt, ri[q]));
                    a.slot_j[slot] = jt; a.slot_p[slot] = pt; a.slot_c[slot] = ct;
                }
            }
        }
        bids += na;
        __syncthreads();
        for (int slot = tid; slot < na; slot += WT) {
            const int jt = ld_sc1(a.slot_j + slot);
            if (jt < 0) continue;                                // retired: stays free, bids no more
            const int i = ld_sc1(A + slot);
            if (bid_won(ld_sc1(a.bid + jt), i)) {
                const int i0 = cx.getcs(jt);
                cx.apply(i, jt, ld_sc1(a.slot_p + slot), ld_sc1(a.slot_c + slot), i0);
                if (i0 >= 0) B[atomicAdd(&s.cnt[cur ^ 1], 1)] = i0;
            } else {
                B[atomicAdd(&s.cnt[cur ^ 1], 1)] = i;
            }
        }
        if (tid == 0) {
            s.cnt[cur] = 0;
            if (a.aug_seg == 0 && a.seg_sync && round > round0) {     // (s.dense: complete since the barrier behind the bids)
                if (s.dense - dense0 >= a.arr_waste) { s.pause = 1; if (!announced) atomicAdd(a.seg_sync, 1); announced = true; }
                else if (a.seg_quorum > 0 && ld_sc1(a.seg_sync) >= a.seg_quorum) s.pause = 1;
            }
        }
        cur ^= 1;
        { int32_t *t_ = A; A = B; B = t_; }
        round++;
        __syncthreads();
    }
    t_list = wall_clock64() - t_start;
    n_list = (headed && h->launches > 0) ? h->list_rounds + (round - round0) : round;      // (the machine's rounds count as list rounds)
    const long long t_chain0 = wall_clock64();
    // ================= CHAIN rounds: wave w holds the rows of slots q * 16 + w =================
    int left = na;                                               // rows still active when the rounds end
    if (!paused && !no_more && na > 0 && na <= ASL && round < a.max_rounds) {
        int my[ACS], jt[ACS], i0[ACS];
        uint32_t col[ACS], ncol[ACS];
        float val[ACS], nval[ACS], pt[ACS], ct[ACS];
#pragma unroll
        for (int q = 0; q < ACS; q++) {
            const int e = q * WNW + w;
            my[q] = e < na ? uni(ld_sc1(A + e)) : -1;
            col[q] = COLSENT; val[q] = 0.0f; ncol[q] = COLSENT; nval[q] = 0.0f;
            if (my[q] >= 0) { col[q] = a.cache_col[(int64_t)my[q] * KC + lane]; val[q] = a.cache_val[(int64_t)my[q] * KC + lane]; }
        }
        int dealt = na;
#ifdef CYTO_WIDE_PROF
        long long tp[5] = {0, 0, 0, 0, 0}, tm = wall_clock64();
#define CH_LAP(k) { const long long now_ = wall_clock64(); tp[k] += now_ - tm; tm = now_; }
#endif
        for (;;) {
#ifdef CYTO_WIDE_PROF
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            CH_LAP(0)
#endif
#pragma unroll
            for (int q = 0; q < ACS; q++) {
                jt[q] = -2; i0[q] = -1; pt[q] = 0.0f; ct[q] = 0.0f;
                if (my[q] >= 0) {
                    cx.bid_of(my[q], w, col[q], val[q], jt[q], pt[q], ct[q], i0[q]);
                    if (i0[q] >= 0) { ncol[q] = a.cache_col[(int64_t)i0[q] * KC + lane]; nval[q] = a.cache_val[(int64_t)i0[q] * KC + lane]; }   // in flight across the barrier
                    if (jt[q] < 0 && lane == 0) atomicAdd(&s.retired, 1);
                }
                if (lane == 0) { s.sm_j[q * WNW + w] = jt[q]; s.sm_i[q * WNW + w] = my[q]; s.sm_p[q * WNW + w] = pt[q]; }
            }
            bids += na;
#ifdef CYTO_WIDE_PROF
            CH_LAP(1)
#endif
            lds_barrier();
#ifdef CYTO_WIDE_PROF
            CH_LAP(2)
#endif
            int nact = 0;
            {
                const int oj = s.sm_j[lane], oi = s.sm_i[lane];
                const float op = s.sm_p[lane];
#pragma unroll
                for (int q = 0; q < ACS; q++) {
                    if (my[q] < 0) continue;
                    if (jt[q] < 0) { my[q] = -1; continue; }      // retired
                    const bool better = oj == jt[q] && lane != q * WNW + w && (op < pt[q] || (op == pt[q] && oi < my[q]));
                    if (!__ballot(better)) {
                        if (lane == 0) cx.apply(my[q], jt[q], pt[q], ct[q], i0[q]);
                        my[q] = i0[q]; col[q] = ncol[q]; val[q] = nval[q];     // the displaced owner bids in the next round (or nobody)
                    }
                    nact += my[q] >= 0;
                }
            }
            if (lane == 0) s.wcnt[w] = nact;
            round++;
            // (a full-row bid with its cache refresh holds up the whole round here: 16 waves wait for the one that sweeps -- a
            //  quarter of the list regime's allowance, then the rows go back to the list and the rounds pause for fresh caches)
            if (tid == 0 && a.aug_seg == 0 && a.seg_sync) {
                if (s.dense - dense0 >= (a.arr_waste + 3) / 4) { s.pause = 1; if (!announced) atomicAdd(a.seg_sync, 1); announced = true; }
                else if (a.seg_quorum > 0 && ld_sc1(a.seg_sync) >= a.seg_quorum) s.pause = 1;
            }
#ifdef CYTO_WIDE_PROF
            CH_LAP(3)
#endif
            if (VLDS) lds_barrier();          // prices and owners are exchanged through LDS: the global stores may still be in flight
            else __syncthreads();             // ... through L2: the round's stores are acknowledged before anyone bids again
            na = 0;
#pragma unroll
            for (int k = 0; k < WNW; k++) na += s.wcnt[k];
            na = uni(na);
            left = na;
#ifdef CYTO_WIDE_PROF
            CH_LAP(4)
#endif
            if (na == 0 || round >= a.max_rounds) break;
            if (uni(s.pause)) {
                cur = (int)(round & 1);                                // the list the next launch reads: by the round's parity
                A = cur ? a.act1 : a.act0;
                if (tid == 0) s.cnt[cur] = 0;
                lds_barrier();
#pragma unroll
                for (int q = 0; q < ACS; q++)
                    if (my[q] >= 0 && lane == 0) st_sc1(A + atomicAdd(&s.cnt[cur], 1), (int32_t)my[q]);
                paused = true;
                break;
            }
            if (na * 2 <= dealt && dealt > WNW) {
                // half of the rows have dropped out: deal the rest out again, round-robin over the waves
#pragma unroll
                for (int q = 0; q < ACS; q++)
                    if (my[q] >= 0 && lane == 0) s.deal[atomicAdd(&s.ndeal, 1)] = my[q];
                lds_barrier();
#pragma unroll
                for (int q = 0; q < ACS; q++) {
                    const int e = q * WNW + w;
                    my[q] = e < na ? uni(s.deal[e]) : -1;
                    if (my[q] >= 0) { col[q] = a.cache_col[(int64_t)my[q] * KC + lane]; val[q] = a.cache_val[(int64_t)my[q] * KC + lane]; }
                }
                dealt = na; n_deal++;
                lds_barrier();
                if (tid == 0) s.ndeal = 0;
            }
        }
#ifdef CYTO_WIDE_PROF
        if (tid == 0) {     // the overlay (lap_dev.h, WT_*): the last of the five parts lands in WT_PAR_BATCHES and in WT_PAR_DISCARDED
            long long *tmr = lap_status(a.misc)->timers;
            for (int k = 0; k < 5; k++) tmr[WT_ARR_LAUNCHES + k > WT_PAR_BATCHES ? WT_PAR_BATCHES : WT_ARR_LAUNCHES + k] = tp[k];
            tmr[WT_PAR_DISCARDED] = tp[4];
        }
#endif
    }
    __syncthreads();
    t_chain = wall_clock64() - t_chain0; n_chain = round - n_list;
    const long long t_tail0 = wall_clock64();
    // ---- the rows still free, in ascending order, for the augmentation ----
    int numfree = 0;
    for (int i0 = 0; i0 < n; i0 += WT) {
        const int i = i0 + tid;
        const bool fr = i < n && ld_sc1(a.rowsol + i) < 0;
        const uint64_t m = __ballot(fr);
        if (lane == 0) s.wcnt[w] = __popcll(m);
        __syncthreads();
        int pre = 0, tot = 0;
#pragma unroll
        for (int k = 0; k < WNW; k++) { const int c = s.wcnt[k]; if (k < w) pre += c; tot += c; }
        if (fr) a.freerows[numfree + pre + __popcll(m & lanemask_lt())] = i;
        numfree += tot;
        __syncthreads();
    }
    if (tid == 0) {
        long long *ctr = lap_status(a.misc)->counters;
        long long *wc = lap_status(a.misc)->wide;
        ctr[C_ARR] = bids; ctr[C_FREE_CR] = free_cr; ctr[C_FREE_A1] = numfree; ctr[C_FREE_A2] = numfree;
        wc[WC_ROUNDS] = round; wc[WC_BIDS] = bids; wc[WC_RETIRED] = s.retired; wc[WC_ACTIVE_LEFT] = left;
        wc[WC_FREE_ARR] = numfree; wc[WC_DENSE_ARR] = s.dense;
        lap_status(a.misc)->numfree = numfree;
        long long *tmr = lap_status(a.misc)->timers;
        tmr[WT_LIST_ROUNDS] = n_list; tmr[WT_LIST_TICKS] += t_list; tmr[WT_CHAIN_ROUNDS] = n_chain; tmr[WT_CHAIN_TICKS] += t_chain;
        tmr[WT_DEALS] = n_deal; tmr[WT_ARR_TAIL_TICKS] = wall_clock64() - t_tail0;
        // the state for the next launch, if the rounds paused (cur == round & 1: both flip together)
        h->started = 1; h->round = round; h->bids = bids; h->retired = s.retired; h->dense = s.dense; h->cnt[cur] = paused ? na : 0;
        h->cnt[cur ^ 1] = 0; h->free_cr = free_cr; h->done = paused ? 0 : 1; h->launches += 1; h->list_rounds = n_list;
#ifndef CYTO_WIDE_PROF
        tmr[WT_ARR_LAUNCHES] = h->launches;
#endif
        // bit 0: the rounds paused for fresh row caches; bit 1: the row reduction hardly ever had to read a full row (<= n / 64 bids):
        // the caches are evidently in good shape, the driver skips the rebuild before the searches (floors stay valid bounds while
        // prices only fall; n = 50 000: 3.3 of 50 ms)
        if (a.seg_sync) a.seg_sync[1 + blockIdx.x] = (paused ? 1 : 0) | ((!paused && s.dense <= n / 64) ? 2 : 0);
    }
}

int wide_launch_rt(const WideArgs *d_args, int nb, int n, hipStream_t stream) {
    const int blocks = std::max(1, std::min((n + RTB / 64 - 1) / (RTB / 64), 2048 / std::max(1, std::min(nb, 8))));
    hipLaunchKernelGGL(wide_rt, dim3(blocks, nb), dim3(RTB), 0, stream, d_args);
    CYTO_HIP(hipGetLastError());
    return CYTO_OK;
}

int wide_launch_arr(const WideArgs *d_args, int nb, int n, hipStream_t stream, int wipe_every, bool resume, int32_t *d_sync,
                    int (*rebuild)(void *ctx, const int32_t *flags), void *ctx, const WideArgs *direct) {
    // The phase machine on the whole chip (one launch per round), in groups of launches: after a group the driver asks which problems
    // are not through (one small read) and rebuilds the row caches of those whose floors have gone stale; then wide_arr -- one
    // workgroup per problem -- for the chain rounds of the problems that did not scale (<= 64 active rows) and the free lists.
    // resume: wide_arr's chain rounds paused for fresh row caches -- it alone picks them up
    // (wipe: launches PER WORD BUFFER between two resets of its bid words -- the words' 12-bit tag counts launches since the reset)
    const int wipe = std::max(1, std::min(wipe_every > 0 ? wipe_every : 1024, 2047));
    int rc;
    if (n >= 2 && !resume) {
        // a wave per bid while the chip has room for them (a bid is a chain of L2 round trips: what counts is how many are in flight)
        // (at most 1 024 workgroups: late in a phase a few hundred rows bid and a launch is mostly the dispatch of workgroups that find
        //  nothing to do -- gpurun_out/r05i, the phase with 256 / 512 / 1 024 / 2 048 workgroups: 20 000^2 6.64 / 6.43 / 6.44 / 7.18 ms,
        //  50 000^2 19.1 / 18.3 / 18.3 / 19.3 ms, few-cell-type 20 000^2 27.7 / 24.4 / 24.2 / 25.1 ms, a 10 000-cell chunk 12.4 / 11.5 / 11.3 / 12.3 ms)
        int bid_total = 4096;
        if (CYTO_KNOB("CYTO_BID_TOTAL").set) bid_total = std::max(64, CYTO_KNOB("CYTO_BID_TOTAL").value);        // (developer knob, read once per process: tools/exp/bid_grid_batch_ab.sh)
        int bx = std::max(1, std::min((n + HEADB / 64 - 1) / (HEADB / 64), std::min(1024, std::max(64, bid_total / std::max(1, nb)))));
        if (CYTO_KNOB("CYTO_BID_GRID").set) bx = std::max(1, std::min(bx, CYTO_KNOB("CYTO_BID_GRID").value));        // (developer knob, read once per process: tools/exp/bid_grid_ab.sh)
        const int bxr = std::max(1, std::min((n + HEADB - 1) / HEADB, 2048 / std::max(1, std::min(nb, 16))));
        // (quads of a full-row bid's sweep in flight per lane: developer knob CYTO_BID_UNROLL, tools/exp/bid_unroll_ab.sh)
        const int unroll = CYTO_KNOB("CYTO_BID_UNROLL").set ? CYTO_KNOB("CYTO_BID_UNROLL").value : SC_UNROLL;
        // (one problem: the control block and the machine's arrays are kernel arguments -- one dependent load less per launch)
        char *sc_direct = nullptr, *scx_direct = nullptr;
        if (nb == 1 && direct) { sc_direct = direct->sc; scx_direct = direct->scx; }
        using RoundK = void (*)(const WideArgs *, int, int, char *, char *, int *, int);
        RoundK roundk = sc_direct ? (unroll == 8 ? (RoundK)wide_sc_round<8, true> : unroll == 4 ? (RoundK)wide_sc_round<4, true> : unroll == 3 ? (RoundK)wide_sc_round<3, true> : (RoundK)wide_sc_round<2, true>)
                                  : (unroll == 8 ? (RoundK)wide_sc_round<8, false> : unroll == 4 ? (RoundK)wide_sc_round<4, false> : unroll == 3 ? (RoundK)wide_sc_round<3, false> : (RoundK)wide_sc_round<2, false>);
        if ((rc = set_max_dynamic_lds(reinterpret_cast<const void *>(roundk)))) return rc;
        hipLaunchKernelGGL(wide_sc_init, dim3(bxr, nb), dim3(HEADB), 0, stream, d_args);
        // The driver never waits for the chip: the launches' first thread reports into pinned host memory which launch is under way,
        // how many machines are through and who wants fresh row caches; the driver keeps a bounded number of launches queued ahead of
        // the one under way (launches of a machine that is through return at once) and stops when every machine is through.
        PinnedInts t_hs;                                              // (from the pool; usable again once the launches queued below have run)
        if ((rc = t_hs.ensure(4 + (size_t)nb, stream))) return rc;
        volatile int *hs = t_hs.p;
        for (int k = 0; k < 4 + nb; k++) hs[k] = 0;
        std::vector<int32_t> seen((size_t)nb, 0), flags((size_t)nb, 0);
        // (developer knobs: launches queued ahead -- 8 / 16 / 48 / 128: 20 000^2 6.32 / 6.39 / 6.47 / 6.57 ms, gpurun_out/r05k; up to how many
        //  bids a launch gives every bid a wave of its own -- 512 / 1 024 / 2 048 / 4 096: 50 000^2 18.2 / 18.0 / 17.9 / 22.0 ms)
        const int ahead = CYTO_KNOB("CYTO_SC_AHEAD").set ? std::max(2, CYTO_KNOB("CYTO_SC_AHEAD").value) : 16;
        const int small_max = CYTO_KNOB("CYTO_SC_SMALL").set ? CYTO_KNOB("CYTO_SC_SMALL").value : SC_SMALL;
        int L = 0;
        // a NO-PROGRESS timeout: the clock restarts whenever the launch under way changes (a slow but advancing run -- counter passes of
        // a profiler, a GPU shared by several ranks -- is not an error); before an error return the stream is drained, because the
        // launches still queued read the buffers the caller releases and report into the pinned block
        SpinWait sw;
        int seen_launch = 0;
        auto t_progress = std::chrono::steady_clock::now();
        auto fail = [&]() -> int { (void)hipStreamSynchronize(stream); return CYTO_ERR_INTERNAL; };
        for (;;) {
            if (hs[1] >= nb) break;
            const int under_way = hs[0];
            if (under_way != seen_launch) { seen_launch = under_way; t_progress = std::chrono::steady_clock::now(); sw.reset(); }
            if (L - under_way >= ahead) {
                sw.pause();
                if ((sw.polls & 0xFFFF) == 0) {
                    if (hipStreamQuery(stream) != hipErrorNotReady && hs[1] < nb && L - hs[0] >= ahead) return fail();      // (the queue has drained and nobody reported: a launch failed)
                    if (std::chrono::steady_clock::now() - t_progress > std::chrono::seconds(120)) return fail();
                }
                continue;
            }
            bool want = false;
            for (int b = 0; b < nb; b++) { const int w_ = hs[4 + b]; flags[(size_t)b] = w_ != seen[(size_t)b] ? 1 : 0; seen[(size_t)b] = w_; want = want || flags[(size_t)b]; }
            if (want && rebuild && (rc = rebuild(ctx, flags.data()))) { (void)hipStreamSynchronize(stream); return rc; }
            for (int g = 0; g < 8; g++, L++) {
                if ((L >> 1) > 0 && (L >> 1) % wipe == 0) hipLaunchKernelGGL(wide_sc_wipe, dim3(bxr, nb), dim3(HEADB), 0, stream, d_args, L);
                hipLaunchKernelGGL(roundk, dim3(bx, nb), dim3(HEADB), SC_SHARED_BYTES, stream, d_args, L, n, sc_direct, scx_direct, t_hs.p, small_max);
            }
            if (L > (1 << 22)) return fail();                          // (every phase is bounded: cannot happen)
        }
        (void)d_sync;
        hipLaunchKernelGGL(wide_sc_finish, dim3(nb), dim3(64), 0, stream, d_args, L);
        CYTO_HIP(hipGetLastError());
    }
    const bool vlds = wide_arr_vlds(n), clds = wide_arr_clds(n);
    void (*k)(const WideArgs *) = vlds ? wide_arr<true, true> : clds ? wide_arr<false, true> : wide_arr<false, false>;
    if ((rc = set_max_dynamic_lds(reinterpret_cast<const void *>(k)))) return rc;
    hipLaunchKernelGGL(k, dim3(nb), dim3(WT), wide_arr_lds_bytes(n, vlds, clds), stream, d_args);
    CYTO_HIP(hipGetLastError());
    return CYTO_OK;
}

}  // namespace cyto
