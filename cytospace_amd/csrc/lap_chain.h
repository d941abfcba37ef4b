// lap_chain.h -- what the float32 driver with its streaming kernels (lap_jv.hip), the float32 chain solver (lap_chain_f32.hip) and the
// float64 solver (lap_f64.hip) share: vector types and the row indirection, the column reduction's first two kernels, the
// workgroup-wide reductions of the 1024-thread kernels, agent-scope accesses, and the host functions lap_jv.hip and lap_f64.hip call
// in each other.  Device code here is templates and inline functions only (a plain __global__ function in a header that several
// files include would be defined more than once).
#pragma once
#include "cyto_common.h"
#include "lap_dev.h"
#include <math.h>

namespace cyto {

constexpr int BLOCK = 1024;
constexpr int NW = BLOCK / 64;

template <typename T> struct VecOf;
template <> struct VecOf<float> { using type = float4; static constexpr int W = 4; };
template <> struct VecOf<double> { using type = double2; static constexpr int W = 2; };

// Row indirection (first half): CytoSPACE repeats every spot row slots[s] times
// (linear_assignment_solvers.py:63-66).  With a row map the cost holds every DISTINCT row once (S_u x C) and LAP row i reads
// row rowmap[i]; without one (nullptr) row i is row i.  RBASE gives callees that compute `base + i * ld` themselves a base that
// lands on the mapped row.
__device__ __forceinline__ int64_t row_off(const int32_t *__restrict__ rowmap, int i, int64_t ld) {
    return (int64_t)(rowmap ? rowmap[i] : i) * ld;
}
#define RBASE(cost_, rowmap_, i_, ld_) ((cost_) + (row_off((rowmap_), (i_), (ld_)) - (int64_t)(i_) * (ld_)))

template <typename T> __device__ __forceinline__ T vec_get(const typename VecOf<T>::type &x, int e);
template <> __device__ __forceinline__ float vec_get<float>(const float4 &x, int e) {
    return e == 0 ? x.x : e == 1 ? x.y : e == 2 ? x.z : x.w;
}
template <> __device__ __forceinline__ double vec_get<double>(const double2 &x, int e) { return e == 0 ? x.x : x.y; }

__device__ __forceinline__ bool memcmp_neq(float a, float b) { return __float_as_uint(a) != __float_as_uint(b); }
__device__ __forceinline__ bool memcmp_neq(double a, double b) { return __double_as_longlong(a) != __double_as_longlong(b); }

// ------------------------------------------------------------------------------------------
// COLUMN REDUCTION
// ------------------------------------------------------------------------------------------
// Partial column minima over a block of rows.  Lane owns VW consecutive columns; each row is one
// 16-byte load per lane (a wave reads 1 KiB contiguous).  Strict '<' while rows ascend keeps the
// lowest row index on ties, exactly like the oracle's row-wise sweep.
template <typename T>
__global__ __launch_bounds__(256) void colred_partial(int n, int64_t ld, const T *__restrict__ cost,
                                                      int rows_per_block, T *__restrict__ pmin,
                                                      int32_t *__restrict__ parg, int *__restrict__ nonfinite,
                                                      int nrows, const int32_t *__restrict__ ulist,
                                                      const int32_t *__restrict__ ufirst) {
    // nrows rows are swept (n without a row map).  With one: the k-th DISTINCT row that is in use is row ulist[k] of the
    // cost and stands for the LAP rows starting at ufirst[k] (ascending in k) -- the lowest of them is what a tie keeps.
    using V = typename VecOf<T>::type;
    constexpr int VW = VecOf<T>::W;
    const int q = blockIdx.x * 256 + threadIdx.x;  // vector-column index
    const int col0 = q * VW;
    const int r0 = blockIdx.y * rows_per_block;
    const int r1 = min(nrows, r0 + rows_per_block);
    if (col0 >= n) return;
    T mn[VW];
    int32_t arg[VW];
    bool bad = false;
#pragma unroll
    for (int e = 0; e < VW; e++) { mn[e] = (T)INFINITY; arg[e] = ufirst ? ufirst[min(r0, nrows - 1)] : r0; }
    const int64_t stride = ld / VW;
#pragma unroll 4
    for (int r = r0; r < r1; r++) {
        const V x = *(reinterpret_cast<const V *>(cost + (int64_t)(ulist ? ulist[r] : r) * ld) + q);
        const int32_t rid = ufirst ? ufirst[r] : r;
#pragma unroll
        for (int e = 0; e < VW; e++) {
            const T xe = vec_get<T>(x, e);
            if (col0 + e < n) bad |= !__builtin_isfinite(xe);
            if (xe < mn[e]) { mn[e] = xe; arg[e] = rid; }
        }
    }
    (void)stride;
#pragma unroll
    for (int e = 0; e < VW; e++) {
        if (col0 + e < n) {
            pmin[(int64_t)blockIdx.y * n + col0 + e] = mn[e];
            parg[(int64_t)blockIdx.y * n + col0 + e] = arg[e];
        }
    }
    if (bad) atomicOr(nonfinite, 1);
}

// Combine the row blocks in ascending order; v[j] = column minimum, imin[j] = its lowest row.
// "Columns are claimed from the last to the first, the first claim of a row wins":
// rowsol[i] = max{ j : imin[j] == i }, matches[i] = #{ j : imin[j] == i }.
template <typename T>
__global__ void colred_finish(int n, int nblocks, const T *__restrict__ pmin, const int32_t *__restrict__ parg,
                              T *__restrict__ v, int32_t *__restrict__ imin, int32_t *rowsol, int32_t *matches) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    T mn = pmin[j];
    int32_t arg = parg[j];
    for (int b = 1; b < nblocks; b++) {
        const T x = pmin[(int64_t)b * n + j];
        if (x < mn) { mn = x; arg = parg[(int64_t)b * n + j]; }
    }
    v[j] = mn;
    imin[j] = arg;
    atomicMax(&rowsol[arg], j);
    atomicAdd(&matches[arg], 1);
}

// ------------------------------------------------------------------------------------------
// Workgroup-wide reductions.  Values are reduced with wave64 shuffles, then the 16 wave
// partials go through LDS once; every lane ends up with the result, so all threads can run
// the (identical) scalar control logic without a broadcast.  `par` alternates 0/1 between
// consecutive reductions so one barrier per reduction suffices.
// ------------------------------------------------------------------------------------------
template <typename T> struct Top2 {
    T u1; uint32_t k1; T a1;  // lexicographic minimum (value, key) and an attached payload
    T u2; uint32_t k2;        // lexicographic minimum excluding k1
};

template <typename T> __device__ __forceinline__ bool lex_less(T a, uint32_t ka, T b, uint32_t kb) {
    return (a < b) || (a == b && ka < kb);
}

template <typename T> __device__ __forceinline__ void top2_push(Top2<T> &t, T h, uint32_t key, T aux) {
    if (lex_less(h, key, t.u1, t.k1)) {
        t.u2 = t.u1; t.k2 = t.k1;
        t.u1 = h; t.k1 = key; t.a1 = aux;
    } else if (lex_less(h, key, t.u2, t.k2)) {
        t.u2 = h; t.k2 = key;
    }
}

template <typename T> __device__ __forceinline__ void top2_merge(Top2<T> &a, const Top2<T> &b) {
    if (lex_less(b.u1, b.k1, a.u1, a.k1)) {
        T nu2; uint32_t nk2;
        if (lex_less(a.u1, a.k1, b.u2, b.k2)) { nu2 = a.u1; nk2 = a.k1; } else { nu2 = b.u2; nk2 = b.k2; }
        a.u1 = b.u1; a.k1 = b.k1; a.a1 = b.a1; a.u2 = nu2; a.k2 = nk2;
    } else if (lex_less(b.u1, b.k1, a.u2, a.k2)) {
        a.u2 = b.u1; a.k2 = b.k1;
    }
}

template <typename T> struct RedScratch {
    T u1[2][NW]; T a1[2][NW]; T u2[2][NW];
    uint32_t k1[2][NW]; uint32_t k2[2][NW];
    int scan[2][NW];
};

template <typename T> __device__ __forceinline__ Top2<T> top2_shfl_xor(const Top2<T> &t, int off) {
    Top2<T> o;
    o.u1 = __shfl_xor(t.u1, off); o.k1 = __shfl_xor(t.k1, off); o.a1 = __shfl_xor(t.a1, off);
    o.u2 = __shfl_xor(t.u2, off); o.k2 = __shfl_xor(t.k2, off);
    return o;
}

template <typename T> __device__ __forceinline__ Top2<T> wg_top2(Top2<T> t, RedScratch<T> &s, int &par) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) top2_merge(t, top2_shfl_xor(t, off));
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) { s.u1[par][w] = t.u1; s.k1[par][w] = t.k1; s.a1[par][w] = t.a1; s.u2[par][w] = t.u2; s.k2[par][w] = t.k2; }
    __syncthreads();
    const int l = lane & (NW - 1);
    Top2<T> r;
    r.u1 = s.u1[par][l]; r.k1 = s.k1[par][l]; r.a1 = s.a1[par][l]; r.u2 = s.u2[par][l]; r.k2 = s.k2[par][l];
#pragma unroll
    for (int off = NW / 2; off >= 1; off >>= 1) top2_merge(r, top2_shfl_xor(r, off));
    par ^= 1;
    return r;
}

// lexicographic (val, key) minimum with payload; cheaper than the full top-2
template <typename T> struct Min1 { T u; uint32_t k; T a; };

template <typename T> __device__ __forceinline__ Min1<T> wg_min1(Min1<T> t, RedScratch<T> &s, int &par) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const T ou = __shfl_xor(t.u, off); const uint32_t ok = __shfl_xor(t.k, off); const T oa = __shfl_xor(t.a, off);
        if (lex_less(ou, ok, t.u, t.k)) { t.u = ou; t.k = ok; t.a = oa; }
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) { s.u1[par][w] = t.u; s.k1[par][w] = t.k; s.a1[par][w] = t.a; }
    __syncthreads();
    const int l = lane & (NW - 1);
    Min1<T> r; r.u = s.u1[par][l]; r.k = s.k1[par][l]; r.a = s.a1[par][l];
#pragma unroll
    for (int off = NW / 2; off >= 1; off >>= 1) {
        const T ou = __shfl_xor(r.u, off); const uint32_t ok = __shfl_xor(r.k, off); const T oa = __shfl_xor(r.a, off);
        if (lex_less(ou, ok, r.u, r.k)) { r.u = ou; r.k = ok; r.a = oa; }
    }
    par ^= 1;
    return r;
}

// exclusive prefix sum over the workgroup (thread order); returns offset, *total = sum
template <typename T> __device__ __forceinline__ int wg_exscan(int x, RedScratch<T> &s, int &par, int *total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = x;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int y = __shfl_up(inc, off);
        if (lane >= off) inc += y;
    }
    if (lane == 63) s.scan[par][w] = inc;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < NW; i++) {
        const int c = s.scan[par][i];
        if (i < w) base += c;
        tot += c;
    }
    par ^= 1;
    *total = tot;
    return base + inc - x;
}

// agent-scope relaxed accesses: served by L2, never by the scalar cache or a stale L1 line
__device__ __forceinline__ int32_t ld_i32(const int32_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_i32(int32_t *p, int32_t x) {
    __hip_atomic_store(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// lexicographic minimum of 64-bit keys over a wave as two 32-bit all-reduces (value, then the low word
// among the lanes holding that value): much shorter dependency chains than a 64-bit DPP butterfly
__device__ __forceinline__ uint64_t wave_lexmin_u64(uint64_t k) {
    const uint32_t hi = (uint32_t)(k >> 32), lo = (uint32_t)k;
    const uint32_t m = wave_min_u32(hi);
    const uint32_t l = wave_min_u32(hi == m ? lo : 0xFFFFFFFFu);
    return ((uint64_t)m << 32) | l;
}

constexpr int FAST_NMAX = 1 << 18;   // largest n of either precision (the float32 cached-chain path: index arithmetic is 32-bit in bytes per row)

// ------------------------------------------------------------------------------------------
// host side: what lap_jv.hip and lap_f64.hip call in each other
// ------------------------------------------------------------------------------------------
inline const cyto_lap_opts k_default_opts = {};

// lap_jv.hip
int check_opts(const cyto_lap_opts &o);
void info_from_counters(cyto_lap_info *info, int n, const LapStatus &h);
int lap_solve_f32(int n, const float *cost, int64_t ld, int cost_on_device, int32_t *rowsol, int32_t *colsol,
                  float *u, float *v, double *total, cyto_lap_info *info, int device_id, hipStream_t stream,
                  const cyto_lap_opts &opts);
// the column reduction's last kernel (colred_assign): colsol from imin and rowsol
void launch_colred_assign(int n, const int32_t *imin, const int32_t *rowsol, int32_t *colsol, hipStream_t stream);
// float64 -> float32 of a row-major n x n matrix on the device, and the grid of that copy and of its widening twin
inline dim3 matrix_copy_grid(int n) { return dim3((n + 255) / 256 > 64 ? 64 : (n + 255) / 256, n > 32768 ? 32768 : n); }
int narrow_to_f32(int n, int64_t ld_src, const double *src, int64_t ld_dst, float *dst, hipStream_t stream);

// lap_f64.hip
int lap_solve_f64(int n, const double *cost, int64_t ld, int cost_on_device, int32_t *rowsol, int32_t *colsol,
                  double *u, double *v, double *total, cyto_lap_info *info, int device_id, hipStream_t stream,
                  const cyto_lap_opts &opts, const float *warm_prices_host = nullptr);
int lap_polish_f64(int n, const float *cost, int64_t ld, int cost_on_device, const int32_t *rowmap_host, int nu, const float *v32,
                   int32_t *rowsol, int32_t *colsol, float *u, float *v, double *total, double *ms_out, int device_id,
                   hipStream_t stream);

}  // namespace cyto
