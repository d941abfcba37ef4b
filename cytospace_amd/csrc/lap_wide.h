// lap_wide.h -- the interface between the float32 driver (lap_jv.hip) and the wide solver (lap_wide_drv.hip: the driver;
// lap_wide.hip: the searches; lap_wide_rr.hip: the row reduction); the row-cache build and the description of a problem (SolveJob) also serve the float32 chain solver (lap_chain_f32.h).
#pragma once
#include "cyto_common.h"
#include "lap_dev.h"
#include <vector>

namespace cyto {

constexpr int WIDE_PAR_GMAX = 64;      // most searches of one problem at once (cyto_lap_opts.wide_par)

// The row caches of one problem against its prices v (lap_jv.hip: build_row_caches_wave, then replicate_group_caches over the runs of
// identical rows): what both solvers start from, and what the wide solver rebuilds between its launches.  rowlist: build only these
// `count` rows (device memory; any order), or null: all of them.
struct CachePlan {
    int waves = 8, unroll = 4;          // waves per CU, quads in flight per lane
    int stream = 1;                     // 1: the guess-free single sweep (cb_stream); 0: a neighbour's floor as the guess
    int cus = 256;                      // CUs of the device (device_cus)
};
int build_caches(const CachePlan &cp, int n, int64_t ld, const float *cost, const int32_t *rowmap, const float *v, uint32_t *cache_col,
                 float *cache_val, const int32_t *same, hipStream_t stream, const int32_t *rowlist = nullptr, int count = 0);

// One problem of a batch as the float32 driver has set it up (lap_jv.hip: F32Job, private to it, after the column reduction), for
// either solver.  Device memory.  (The slots of fws / iws are named as the wide solver uses them -- lap_wide_dev.h: FWS_*, IWS_* -- ; the chain solver's use: Chain2Args and
// LazyArgs, lap_chain_f32.hip.  first_rows / first_count: the wide solver only.)
struct SolveJob {
    const float *cost; int64_t ld;
    const int32_t *rowmap;              // [n] LAP row i reads stored row rowmap[i], or null
    float *fws;                         // [6n + 16] FWS_V | FWS_U | - | FWS_CASSIGN | FWS_LABEL (2n)
    int32_t *iws;                       // [10n + 16] IWS_ROWSOL | _COLSOL | _MATCHES | _FREEROWS | _ACT0 | _ACT1 | _TOUCHED | _SLOT_J | _BID (2n)
    uint32_t *cache_col; float *cache_val;      // [n][64] row caches
    char *misc;                         // the status block (lap_dev.h: LapStatus)
    const int32_t *same;                // [n] 1 = the row equals the row before it (runs of identical rows), or null
    const int32_t *rowgid;              // [n] the run of identical rows that a row is in, counted from 0 (the chain solver; n >= 2)
    int ngroups;                        // runs of identical rows (n: none)
    DevBuf *state;                      // the solver's own state, the caller's buffers: one (wide), CHAIN_STATE_BUFS (chain); allocated by the solver
    // the first caches came out of the column reduction's pass (lap_jv.hip: fused_fixup) but for these rows; -1: they did not, build all
    const int32_t *first_rows = nullptr; int first_count = -1;
};
struct WidePlan {
    int n;
    long long rounds;                   // cap on the row-reduction rounds (0: none)
    int rebuild, wipe, par;             // cyto_lap_opts.wide_rebuild / wide_wipe / wide_par
    CachePlan cache;
};
// The wide solve of a batch after its column reduction: reduction transfer, row reduction, searches -- one launch per phase for the
// whole batch.  ev_cache_done is recorded behind the first cache build, ev_arr_done behind the row reduction.
int wide_solve_batch(const WidePlan &pl, const std::vector<SolveJob> &jobs, hipStream_t stream, hipEvent_t ev_cache_done,
                     hipEvent_t ev_arr_done);
// the status block of a finished wide solve, once per solve: what the process-wide counters take from it (cyto_wide_embedded_solves)
void wide_note_status(const LapStatus &h);
// the wide solver's fields of cyto_lap_info (the driver has zeroed it)
void wide_info(cyto_lap_info *info, const LapStatus &h);

}  // namespace cyto
