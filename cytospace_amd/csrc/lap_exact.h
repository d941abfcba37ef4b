// lap_exact.h -- the float64 certificate of a float32 solve and the exact option (lap_exact.hip), as the float32 driver (lap_jv.hip)
// runs them behind a solve.
#pragma once
#include "cyto_common.h"
#include "lap_dev.h"
#include <vector>

namespace cyto {

// cyto_lap_opts.exact: edge slots per row of the first emission pass (exact = 1) and the largest slot count a caller may ask for
constexpr int EXACT_SLOTS_DEFAULT = 16, EXACT_SLOTS_MAX = 64;

// The certificate (dual_gap_rows, dual_gap_finish) on the stream.  viol: [n + 3] doubles on the device -- the rows' terms, then their
// sum | max | number of positive ones.  grid: workgroups of four waves, a wave per row.
int certify_launch(int n, int64_t ld, const float *cost, const int32_t *rowmap, const int32_t *rowsol, const float *v, double *viol,
                   int grid, hipStream_t stream);

// One solved problem as the exact option reads it and rewrites its result (the float32 driver's device buffers)
struct ExactView {
    const float *cost; int64_t ld;          // the matrix as the kernels read it (16-byte aligned rows) and its pitch
    const int32_t *rowmap;                  // [n] LAP row i reads stored row rowmap[i], or null
    int32_t *iws;                           // rowsol | colsol | ...
    float *fws;                             // v | u | ...
    LapStatus *st;
};

struct ExactRun {
    int64_t status = 0, edges = 0, free_rows = 0, changed = 0, overflow = 0;   // (cyto_lap_info.exact_*)
    double ms_emit = 0.0, ms_repair = 0.0;
    int cap = 0;
    const double *d_gap = nullptr;          // the certificate's sum on the device (alive while the certificate's buffer is)
    DevBuf b_slots;                         // column (n x cap) | cost (n x cap) | count (n) | c_i,pi (n)
    Events<4> ev;
    std::vector<float> v;                   // the float32 prices: the polish's start when E is over its cap
};

// the first emission pass, queued behind dual_gap_finish (d_gap: the sum it leaves on the device)
int exact_emit(ExactRun &ex, int n, int cap, const ExactView &j, const double *d_gap, int grid, hipStream_t stream);
// after the certificate has arrived: the overflow pass, E on the host, the sparse solve, the repaired result back into the device
// buffers the results are read from (rowsol | colsol, u, total) -- or, over the cap, status 3 (the caller polishes)
int exact_repair(ExactRun &ex, int n, const ExactView &j, double gap, int grid, hipStream_t stream);

}  // namespace cyto
