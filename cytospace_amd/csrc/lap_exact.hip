// lap_exact.hip -- what runs behind a float32 LAP solve when the caller asks how good it is: the float64 certificate
// (cyto_lap_opts.certify: dual_gap_rows / dual_gap_finish) and the exact option built on it (cyto_lap_opts.exact: near_tight_rows emits
// the edges an optimum can use, the host finishes with a sparse solve over them -- repair_sparse, also exported on its own as
// cyto_lap_repair_sparse).  Mostly host code; the float32 driver (lap_jv.hip) calls it through lap_exact.h.
#include "lap_exact.h"
#include <math.h>
#include <cmath>
#include <vector>
#include <algorithm>
#include <functional>
#include <chrono>
#include <new>

namespace cyto {

// ------------------------------------------------------------------------------------------
// The float64 certificate of a float32 solve (cyto_lap_opts.certify).  The solvers compare fl32(c - v): an assigned row sits on a
// minimum of its reduced costs AS ROUNDED, so in exact arithmetic its column can lose to another by a fraction of an ulp -- the
// duals (u_i := c[i][rowsol_i] - v[rowsol_i], v) are feasible to ~1e-9, not exactly.  One more pass over the matrix turns that into a
// PROOF of how far from optimal the assignment can be: with every difference evaluated in float64 (exact for float32 operands
// whose exponents lie within 29 binades of each other),
//     gap = sum_i ( u_i - min_j (c[i][j] - v[j]) )  >=  total - optimum  >=  0
// (lower every u_i to its row's true minimum: the duals become feasible, their objective is total - gap).  gap == 0: the
// assignment is optimal for the float32 matrix in exact arithmetic; an instance whose optimum is unique by more than `gap` has
// exactly these indices whatever the solver's constants.  A wave per row, one sweep; the rows' terms are summed in row order
// (one workgroup, fixed tree): the same bits on every run.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dual_gap_rows(int n, int64_t ld, const float *__restrict__ cost, const int32_t *__restrict__ rowmap,
                                                     const int32_t *__restrict__ rowsol, const float *__restrict__ v,
                                                     double *__restrict__ viol) {
    const int lane = threadIdx.x & 63;
    const int gw = blockIdx.x * 4 + (threadIdx.x >> 6), nw = gridDim.x * 4;
    const int nq = (n + 3) >> 2;
    const float4 *__restrict__ v4 = reinterpret_cast<const float4 *>(v);
    for (int i = gw; i < n; i += nw) {
        const float *__restrict__ row = cost + (int64_t)(rowmap ? rowmap[i] : i) * ld;
        const float4 *__restrict__ r4 = reinterpret_cast<const float4 *>(row);
        double m = INFINITY;
        for (int q0 = lane; q0 < nq; q0 += 64 * 8) {
            float4 x[8], p[8];
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const int q = q0 + 64 * k;
                const bool in = q < nq && q * 4 + 3 < n;                 // (whole quads; the row's last, partial quad below)
                x[k] = in ? r4[q] : make_float4(INFINITY, INFINITY, INFINITY, INFINITY);
                p[k] = in ? v4[q] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
#pragma unroll
            for (int k = 0; k < 8; k++) {
                m = fmin(m, fmin(fmin((double)x[k].x - (double)p[k].x, (double)x[k].y - (double)p[k].y),
                                 fmin((double)x[k].z - (double)p[k].z, (double)x[k].w - (double)p[k].w)));
            }
        }
        if (lane < (n & 3)) { const int c = (n & ~3) + lane; m = fmin(m, (double)row[c] - (double)v[c]); }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) m = fmin(m, __shfl_xor(m, off));
        if (lane == 0) {
            const int j = rowsol[i];
            const double ui = (double)row[j] - (double)v[j];
            viol[i] = ui > m ? ui - m : 0.0;
        }
    }
}
// out[0] = sum (rows in ascending order within a thread, then a fixed tree), out[1] = max, out[2] = rows with a positive term
__global__ __launch_bounds__(1024) void dual_gap_finish(int n, const double *__restrict__ viol, double *__restrict__ out) {
    __shared__ double s_sum[1024], s_max[1024];
    __shared__ int s_cnt[1024];
    const int t = threadIdx.x;
    const int per = (n + 1023) / 1024, lo = t * per, hi = min(n, lo + per);
    double s = 0.0, mx = 0.0; int c = 0;
    for (int i = lo; i < hi; i++) { const double x = viol[i]; s += x; mx = fmax(mx, x); c += x > 0.0; }
    s_sum[t] = s; s_max[t] = mx; s_cnt[t] = c;
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) {
        if (t < w) { s_sum[t] += s_sum[t + w]; s_max[t] = fmax(s_max[t], s_max[t + w]); s_cnt[t] += s_cnt[t + w]; }
        __syncthreads();
    }
    if (t == 0) { out[0] = s_sum[0]; out[1] = s_max[0]; out[2] = (double)s_cnt[0]; }
}

int certify_launch(int n, int64_t ld, const float *cost, const int32_t *rowmap, const int32_t *rowsol, const float *v, double *viol,
                   int grid, hipStream_t stream) {
    hipLaunchKernelGGL(dual_gap_rows, dim3(grid), dim3(256), 0, stream, n, ld, cost, rowmap, rowsol, v, viol);
    hipLaunchKernelGGL(dual_gap_finish, dim3(1), dim3(1024), 0, stream, n, viol, viol + n);
    CYTO_HIP(hipGetLastError());
    return CYTO_OK;
}

// ------------------------------------------------------------------------------------------
// The exact option (cyto_lap_opts.exact; DESIGN.md, "Exact option").  With pi = rowsol and, in float64 (exact as above),
// w_ij = c_ij - v_j and r_ij = w_ij - w_i,pi(i): for any permutation sigma, cost(sigma) - cost(pi) = sum_i r_i,sigma(i), and
// r_ij >= -s_i with gap = sum_i s_i (dual_gap_rows' terms).  An assignment that uses an edge with r > gap costs more than pi,
// so the optimum lies in E = {(i, j) : r_ij <= tau}, tau = gap * (1 + 2^-30) (the slack covers the rounding of the n-term sum
// and of each r; a larger tau only adds edges).  This pass emits E, the host finishes with a sparse solve over it.
//
// A wave per row (row t, or rows[t] of a list): c_i,pi and v_pi first, then one sweep selecting j != pi(i) with r_ij <= tau,
// appended in column order (a ballot per bit of the lane's count, prefix popcounts) as (column, raw float32 cost) at
// base = off ? off[t] : t * cap; the first `cap` are written, the true count and c_i,pi go to count / cpi (when given).  No atomics:
// the same bytes on every run.  The float4 sweep only where the row and v are 16-byte aligned (any ld, any caller pointer: else
// a column per lane).  Reads the gap dual_gap_finish left on the device; gap == 0 (nothing to repair): every wave returns at once.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void near_tight_append(unsigned mask, int j0, const float (&xs)[4], int lane, int cap, int64_t base, int &cnt,
                                                  int32_t *__restrict__ out_col, float *__restrict__ out_val) {
    // mask: the lane's selections among columns j0 ... j0+3.  Three ballots (a lane selects at most 4) give every lane the number
    // of selections in the lanes below it, and the wave's total
    const int cl = __popc(mask);
    const unsigned long long below = (1ull << lane) - 1ull;
    int pre = 0, tot = 0;
#pragma unroll
    for (int b = 0; b < 3; b++) {
        const unsigned long long m = __ballot((cl >> b) & 1);
        pre += __popcll(m & below) << b;
        tot += __popcll(m) << b;
    }
    int p = cnt + pre;
#pragma unroll
    for (int e = 0; e < 4; e++)
        if ((mask >> e) & 1u) {
            if (p < cap) { out_col[base + p] = j0 + e; out_val[base + p] = xs[e]; }
            p++;
        }
    cnt += tot;
}

__global__ __launch_bounds__(256) void near_tight_rows(int nrows, int n, int64_t ld, const float *__restrict__ cost,
                                                       const int32_t *__restrict__ rowmap, const int32_t *__restrict__ rowsol,
                                                       const float *__restrict__ v, const double *__restrict__ gap,
                                                       const int32_t *__restrict__ rows, const int64_t *__restrict__ off, int cap,
                                                       int32_t *__restrict__ out_col, float *__restrict__ out_val,
                                                       int32_t *__restrict__ count, float *__restrict__ cpi) {
    const double g = *gap;
    if (!(g > 0.0)) return;
    const double tau = g * (1.0 + 0x1p-30);
    const int lane = threadIdx.x & 63;
    const int gw = blockIdx.x * 4 + (threadIdx.x >> 6), nw = gridDim.x * 4;
    const int nq = n >> 2;                                           // whole quads; the last n & 3 columns after them
    for (int t = gw; t < nrows; t += nw) {
        const int i = rows ? rows[t] : t;
        const float *__restrict__ row = cost + (int64_t)(rowmap ? rowmap[i] : i) * ld;
        const int jp = rowsol[i];
        const float cp = row[jp];
        const double wp = (double)cp - (double)v[jp];
        const int64_t base = off ? off[t] : (int64_t)t * cap;
        int cnt = 0;                                                 // (wave-uniform)
        const bool vec = ((reinterpret_cast<uintptr_t>(row) | reinterpret_cast<uintptr_t>(v)) & 15) == 0;
        int done = 0;                                                // columns below `done` are swept
        if (vec) {
            const float4 *__restrict__ r4 = reinterpret_cast<const float4 *>(row);
            const float4 *__restrict__ v4 = reinterpret_cast<const float4 *>(v);
            for (int q0 = 0; q0 < nq; q0 += 64 * 8) {
                float4 x[8], p[8];
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    const int q = q0 + 64 * k + lane;
                    const bool in = q < nq;
                    x[k] = in ? r4[q] : make_float4(INFINITY, INFINITY, INFINITY, INFINITY);
                    p[k] = in ? v4[q] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                }
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    const int j0 = 4 * (q0 + 64 * k + lane);
                    const float xs[4] = {x[k].x, x[k].y, x[k].z, x[k].w}, ps[4] = {p[k].x, p[k].y, p[k].z, p[k].w};
                    unsigned mask = 0;
#pragma unroll
                    for (int e = 0; e < 4; e++)          // (padding lanes hold +inf: never selected)
                        mask |= (unsigned)(j0 + e != jp && ((double)xs[e] - (double)ps[e]) - wp <= tau) << e;
                    if (__ballot(mask != 0)) near_tight_append(mask, j0, xs, lane, cap, base, cnt, out_col, out_val);
                }
            }
            done = nq * 4;
        }
        for (int c0 = done; c0 < n; c0 += 64) {                     // (a column per lane: the unaligned case, and the last n & 3 columns)
            const int j = c0 + lane;
            const float xs[4] = {j < n ? row[j] : INFINITY, 0.0f, 0.0f, 0.0f};
            const unsigned mask = (j < n && j != jp && ((double)xs[0] - (double)v[j]) - wp <= tau) ? 1u : 0u;
            if (__ballot(mask != 0)) near_tight_append(mask, j, xs, lane, cap, base, cnt, out_col, out_val);
        }
        if (lane == 0 && count) { count[i] = cnt; cpi[i] = cp; }
    }
}

// the cap on E's edges beyond which the float64 polish runs instead (the host solve and its buffers stay a few hundred MB at most)
static int64_t exact_edge_cap(int n) { return std::max<int64_t>((int64_t)1 << 22, (int64_t)32 * n); }

// ---- the host half of the exact option (cyto_lap_repair_sparse): successive shortest paths over a sparse E ----
// Rows whose own edge is not their cheapest are freed; u_i = min_j r_ij, v = 0 are then feasible and tight on the rows kept (the JV
// invariant: an assigned row sits on a minimum of r_ij - v_j), so each free row in ascending order runs one Dijkstra over the
// columns with those potentials -- a binary heap keyed on (distance, column), equal distances to the lower column -- up to the first
// unassigned column it settles; the settled columns' prices drop by (their distance - the path's), the path is flipped.  What
// comes out is an optimum of the sparse problem; rows off every augmenting path keep their column.  *nfree / *changed: may be null.
static int repair_sparse(int n, const int32_t *rowsol, const int64_t *rp, const int32_t *cols, const double *r, int32_t *out,
                         int64_t *nfree, int64_t *changed) {
    if (n <= 0 || !rowsol || !rp || !cols || !r || !out || rp[0] != 0) return CYTO_ERR_BAD_ARG;
    std::vector<int32_t> rs((size_t)n), cs((size_t)n, -1);
    std::vector<double> ra((size_t)n), v((size_t)n, 0.0);     // ra[i]: r of row i's assigned edge
    std::vector<int32_t> freerows;
    std::vector<char> seen((size_t)n, 0);
    for (int i = 0; i < n; i++) {
        const int j0 = rowsol[i];
        if (j0 < 0 || j0 >= n || seen[(size_t)j0] || rp[i + 1] < rp[i]) return CYTO_ERR_BAD_ARG;
        seen[(size_t)j0] = 1;
        double mn = INFINITY, own = INFINITY;
        for (int64_t e = rp[i]; e < rp[i + 1]; e++) {
            const int j = cols[e];
            if (j < 0 || j >= n || !std::isfinite(r[e])) return CYTO_ERR_BAD_ARG;
            mn = std::min(mn, r[e]);
            if (j == j0) own = std::min(own, r[e]);
        }
        if (own == INFINITY) return CYTO_ERR_BAD_ARG;        // (the starting assignment must lie in E)
        rs[(size_t)i] = j0;
        if (mn < own) { freerows.push_back(i); rs[(size_t)i] = -1; }
        else { cs[(size_t)j0] = i; ra[(size_t)i] = own; }
    }
    // per search: distances and predecessors of the columns it touched (stamped, so nothing is cleared between searches)
    std::vector<double> d((size_t)n), pr((size_t)n);
    std::vector<int32_t> pred((size_t)n), stamp((size_t)n, -1), settled_at((size_t)n, -1);
    std::vector<int32_t> settled;
    typedef std::pair<double, int32_t> Key;
    std::vector<Key> heap;
    auto push = [&](double dist, int32_t j) { heap.emplace_back(dist, j); std::push_heap(heap.begin(), heap.end(), std::greater<Key>()); };
    for (int s = 0; s < (int)freerows.size(); s++) {
        const int f = freerows[(size_t)s];
        heap.clear(); settled.clear();
        auto relax = [&](int i, double base) {               // base: distance of row i's entry minus its own reduced cost
            for (int64_t e = rp[i]; e < rp[i + 1]; e++) {
                const int k = cols[e];
                if (settled_at[(size_t)k] == s) continue;
                const double nd = base + (r[e] - v[(size_t)k]);
                if (stamp[(size_t)k] != s || nd < d[(size_t)k]) {
                    stamp[(size_t)k] = s; d[(size_t)k] = nd; pred[(size_t)k] = i; pr[(size_t)k] = r[e];
                    push(nd, k);
                }
            }
        };
        relax(f, 0.0);
        int end = -1;
        double D = 0.0;
        while (!heap.empty()) {
            std::pop_heap(heap.begin(), heap.end(), std::greater<Key>());
            const Key top = heap.back();
            heap.pop_back();
            const int j = top.second;
            if (settled_at[(size_t)j] == s || top.first != d[(size_t)j]) continue;       // (stale entry)
            settled_at[(size_t)j] = s;
            settled.push_back(j);
            const int i = cs[(size_t)j];
            if (i < 0) { end = j; D = top.first; break; }
            relax(i, top.first - (ra[(size_t)i] - v[(size_t)j]));
        }
        if (end < 0) return CYTO_ERR_INTERNAL;             // (no augmenting path: E held no perfect matching)
        for (int j : settled) v[(size_t)j] += d[(size_t)j] - D;
        for (int j = end;;) {                               // flip the path
            const int i = pred[(size_t)j];
            const int k = rs[(size_t)i];
            cs[(size_t)j] = i; rs[(size_t)i] = j; ra[(size_t)i] = pr[(size_t)j];
            if (i == f) break;
            j = k;
        }
    }
    int64_t ch = 0;
    for (int i = 0; i < n; i++) { ch += rs[(size_t)i] != rowsol[i]; }
    for (int i = 0; i < n; i++) out[i] = rs[(size_t)i];
    if (nfree) *nfree = (int64_t)freerows.size();
    if (changed) *changed = ch;
    return CYTO_OK;
}

// ---- the exact option around the certificate (cyto_lap_opts.exact) ----
// the first emission pass, queued behind dual_gap_finish (d_gap: the sum it leaves on the device)
int exact_emit(ExactRun &ex, int n, int cap, const ExactView &j, const double *d_gap, int grid, hipStream_t stream) {
    int rc;
    ex.cap = cap; ex.d_gap = d_gap;
    if ((rc = ex.ev.create())) return rc;
    const size_t nk = (size_t)n * cap;
    if ((rc = ex.b_slots.alloc(nk * 8 + (size_t)n * 8, stream))) return rc;
    int32_t *s_col = ex.b_slots.as<int32_t>();
    float *s_val = reinterpret_cast<float *>(s_col + nk);
    int32_t *cnt = reinterpret_cast<int32_t *>(s_val + nk);
    float *cpi = reinterpret_cast<float *>(cnt + n);
    CYTO_HIP(hipEventRecord(ex.ev[0], stream));
    hipLaunchKernelGGL(near_tight_rows, dim3(grid), dim3(256), 0, stream, n, n, j.ld, j.cost, j.rowmap, j.iws,
                       j.fws, d_gap, (const int32_t *)nullptr, (const int64_t *)nullptr, cap, s_col, s_val, cnt, cpi);
    CYTO_HIP(hipGetLastError());
    CYTO_HIP(hipEventRecord(ex.ev[1], stream));
    return CYTO_OK;
}

// after the certificate has arrived: the overflow pass, E on the host, the sparse solve, the repaired result back into the device
// buffers the results are read from (rowsol | colsol, u, total) -- or, over the cap, status 3 (the caller polishes)
int exact_repair(ExactRun &ex, int n, const ExactView &j, double gap, int grid, hipStream_t stream) {
    int rc;
    if (!(gap > 0.0)) {                                      // (the emission returned at once)
        ex.status = 1;
        float ms = 0.0f;
        (void)hipEventElapsedTime(&ms, ex.ev[0], ex.ev[1]);
        ex.ms_emit = ms;
        return CYTO_OK;
    }
    const int cap = ex.cap;
    const size_t nk = (size_t)n * cap, nI = (size_t)n * sizeof(int32_t);
    int32_t *s_col = ex.b_slots.as<int32_t>();
    float *s_val = reinterpret_cast<float *>(s_col + nk);
    int32_t *d_cnt = reinterpret_cast<int32_t *>(s_val + nk);
    float *d_cpi = reinterpret_cast<float *>(d_cnt + n);
    int32_t *d_rowsol = j.iws;
    float *d_v = j.fws;
    std::vector<int32_t> cnt((size_t)n), pi((size_t)n);
    std::vector<float> cpi((size_t)n);
    ex.v.resize((size_t)n);
    CYTO_HIP(hipMemcpyAsync(cnt.data(), d_cnt, nI, hipMemcpyDeviceToHost, stream));
    CYTO_HIP(hipMemcpyAsync(cpi.data(), d_cpi, nI, hipMemcpyDeviceToHost, stream));
    CYTO_HIP(hipMemcpyAsync(pi.data(), d_rowsol, nI, hipMemcpyDeviceToHost, stream));
    CYTO_HIP(hipMemcpyAsync(ex.v.data(), d_v, nI, hipMemcpyDeviceToHost, stream));
    CYTO_HIP(hipStreamSynchronize(stream));
    std::vector<int32_t> over_rows;
    std::vector<int64_t> over_off;
    int64_t over_total = 0;
    for (int i = 0; i < n; i++) {
        ex.edges += cnt[(size_t)i];
        if (cnt[(size_t)i] > cap) { over_rows.push_back(i); over_off.push_back(over_total); over_total += cnt[(size_t)i]; }
    }
    ex.overflow = (int64_t)over_rows.size();
    float ms1 = 0.0f, ms2 = 0.0f;
    (void)hipEventElapsedTime(&ms1, ex.ev[0], ex.ev[1]);
    if (ex.edges > exact_edge_cap(n)) { ex.status = 3; ex.ms_emit = ms1; return CYTO_OK; }
    // rows over their slots: emitted again, exactly, into a list of their own
    DevBuf b_list, b_csr;
    std::vector<int32_t> o_col((size_t)over_total);
    std::vector<float> o_val((size_t)over_total);
    if (!over_rows.empty()) {
        const size_t m = over_rows.size();
        if ((rc = b_list.alloc(m * 12 + 16, stream)) || (rc = b_csr.alloc((size_t)over_total * 8, stream))) return rc;
        int64_t *d_off = b_list.as<int64_t>();
        int32_t *d_rows = reinterpret_cast<int32_t *>(d_off + m);
        CYTO_HIP(hipMemcpyAsync(d_off, over_off.data(), m * 8, hipMemcpyHostToDevice, stream));
        CYTO_HIP(hipMemcpyAsync(d_rows, over_rows.data(), m * 4, hipMemcpyHostToDevice, stream));
        int32_t *c_col = b_csr.as<int32_t>();
        float *c_val = reinterpret_cast<float *>(c_col + over_total);
        CYTO_HIP(hipEventRecord(ex.ev[2], stream));
        hipLaunchKernelGGL(near_tight_rows, dim3(std::max(1, std::min(grid, (int)((m + 3) / 4)))), dim3(256), 0, stream, (int)m, n, j.ld, j.cost,
                           j.rowmap, d_rowsol, d_v, ex.d_gap, d_rows, d_off, INT32_MAX, c_col, c_val, (int32_t *)nullptr, (float *)nullptr);
        CYTO_HIP(hipGetLastError());
        CYTO_HIP(hipEventRecord(ex.ev[3], stream));
        CYTO_HIP(hipMemcpyAsync(o_col.data(), c_col, (size_t)over_total * 4, hipMemcpyDeviceToHost, stream));
        CYTO_HIP(hipMemcpyAsync(o_val.data(), c_val, (size_t)over_total * 4, hipMemcpyDeviceToHost, stream));
    }
    std::vector<int32_t> h_col(nk);
    std::vector<float> h_val(nk);
    CYTO_HIP(hipMemcpyAsync(h_col.data(), s_col, nk * 4, hipMemcpyDeviceToHost, stream));
    CYTO_HIP(hipMemcpyAsync(h_val.data(), s_val, nk * 4, hipMemcpyDeviceToHost, stream));
    CYTO_HIP(hipStreamSynchronize(stream));
    if (!over_rows.empty()) (void)hipEventElapsedTime(&ms2, ex.ev[2], ex.ev[3]);
    ex.ms_emit = (double)ms1 + ms2;

    // E in CSR: per row the assignment's own edge (r = 0) first, then the emitted ones, r recomputed with the kernel's operations
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<int64_t> rp((size_t)n + 1);
    std::vector<int32_t> ecol((size_t)(n + ex.edges));
    std::vector<double> er((size_t)(n + ex.edges));
    std::vector<float> ecost((size_t)(n + ex.edges));
    int64_t e = 0;
    for (int i = 0, o = 0; i < n; i++) {
        rp[(size_t)i] = e;
        const int jp = pi[(size_t)i];
        const double wp = (double)cpi[(size_t)i] - (double)ex.v[(size_t)jp];
        ecol[(size_t)e] = jp; er[(size_t)e] = 0.0; ecost[(size_t)e] = cpi[(size_t)i]; e++;
        const int c = cnt[(size_t)i];
        const bool ov = c > cap;
        const int32_t *col = ov ? &o_col[(size_t)over_off[(size_t)o]] : &h_col[(size_t)i * cap];
        const float *val = ov ? &o_val[(size_t)over_off[(size_t)o]] : &h_val[(size_t)i * cap];
        if (ov) o++;
        for (int k = 0; k < c; k++, e++) {
            ecol[(size_t)e] = col[k]; ecost[(size_t)e] = val[k];
            er[(size_t)e] = ((double)val[k] - (double)ex.v[(size_t)col[k]]) - wp;
        }
    }
    rp[(size_t)n] = e;
    std::vector<int32_t> sigma((size_t)n);
    if ((rc = repair_sparse(n, pi.data(), rp.data(), ecol.data(), er.data(), sigma.data(), &ex.free_rows, &ex.changed))) return rc;
    ex.status = 2;
    if (ex.changed) {
        // the total moves by the changed rows' cost differences (float64); u_i = fl32(c_i,sigma(i) - v_sigma(i)) on those rows, v stays
        std::vector<float> u((size_t)n);
        double total = 0.0;
        CYTO_HIP(hipMemcpyAsync(u.data(), d_v + n, nI, hipMemcpyDeviceToHost, stream));
        CYTO_HIP(hipMemcpyAsync(&total, &j.st->total, sizeof total, hipMemcpyDeviceToHost, stream));
        CYTO_HIP(hipStreamSynchronize(stream));
        double delta = 0.0;
        for (int i = 0; i < n; i++) {
            const int js = sigma[(size_t)i];
            if (js == pi[(size_t)i]) continue;
            float cs = 0.0f;
            for (int64_t q = rp[(size_t)i]; q < rp[(size_t)i + 1]; q++) if (ecol[(size_t)q] == js) { cs = ecost[(size_t)q]; break; }
            delta += (double)cs - (double)cpi[(size_t)i];
            u[(size_t)i] = cs - ex.v[(size_t)js];
        }
        total += delta;
        std::vector<int32_t> both((size_t)2 * n);
        for (int i = 0; i < n; i++) { both[(size_t)i] = sigma[(size_t)i]; both[(size_t)n + sigma[(size_t)i]] = i; }
        CYTO_HIP(hipMemcpyAsync(d_rowsol, both.data(), 2 * nI, hipMemcpyHostToDevice, stream));
        CYTO_HIP(hipMemcpyAsync(d_v + n, u.data(), nI, hipMemcpyHostToDevice, stream));
        CYTO_HIP(hipMemcpyAsync(&j.st->total, &total, sizeof total, hipMemcpyHostToDevice, stream));
        CYTO_HIP(hipStreamSynchronize(stream));
    }
    ex.ms_repair = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return CYTO_OK;
}

}  // namespace cyto

extern "C" {

// the host half of cyto_lap_opts.exact on its own (no device): the test suite pins it against an independent exact solver
int cyto_lap_repair_sparse(int n, const int32_t *rowsol, const int64_t *row_ptr, const int32_t *cols, const double *r, int32_t *rowsol_out) {
    try {
        return cyto::repair_sparse(n, rowsol, row_ptr, cols, r, rowsol_out, nullptr, nullptr);
    } catch (const std::bad_alloc &) {
        return CYTO_ERR_NOMEM;
    } catch (...) {
        return CYTO_ERR_INTERNAL;
    }
}

}  // extern "C"
