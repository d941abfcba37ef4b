// resident.hip -- a genes x cells table that stays in HBM between the stages of main_cytospace: the gather that
// turns "these rows, these columns, this element type" of a resident table into the matrix the next stage reads (cyto_select), the
// one streaming pass that tells which element type holds the view exactly (cyto_value_range), and the host hook of the predicate
// both share (cyto_select_check; select_exact.h).
//
// cyto_select is a bandwidth kernel.  Lanes run along the DESTINATION columns, so every store instruction of a wave writes one
// contiguous run of a destination row.  Without a column list the loads are contiguous too, and where the bases and leading
// dimensions allow, a lane moves 16 bytes of the source per load (two int64 / float64 words, four float32, eight uint16) and stores
// its elements with the widest store their size gives (up to 16 bytes).  With a column list a lane reads the one word its column
// names: within a row these are scattered 8-byte reads, served by L2 where columns repeat or lie close (a sampled cell list does
// both) -- the row's words are read once from HBM either way, by cache line.  Rows are whole workgroups' work (blockIdx.y strides
// over them), so a row list costs one scalar load per row.  Every offset is 64-bit: G * ld passes 2^31 at real sizes.
#include "cyto_common.h"
#include "select_exact.h"

#include <algorithm>
#include <limits>
#include <vector>

namespace {

using namespace cyto;

constexpr int WG = 256;
constexpr int MAX_ROW_BLOCKS = 4096;        // blockIdx.y of the select launch (rows beyond it: the stride loop)
constexpr int RANGE_ROW_BLOCKS = 256;       // ... of the range launch, whose every workgroup leaves one partial result

template <typename T, int N> struct alignas(sizeof(T) * N <= 16 ? sizeof(T) * N : 16) Vec {
    T v[N];
};

__device__ inline int64_t wave_sum(int64_t x) {
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
}

// One lane: VEC consecutive destination columns (VEC > 1 only without a column list and with aligned rows: the host decides).
template <typename TS, typename TD, int VEC>
__global__ __launch_bounds__(WG) void select_kernel(const TS *__restrict__ src, int64_t ld_src, const int64_t *__restrict__ rows, int64_t Gs,
                                                    const int64_t *__restrict__ cols, int64_t Cs, TD *__restrict__ dst, int64_t ld_dst,
                                                    unsigned long long *inexact) {
    const int64_t j0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * VEC;
    int64_t bad = 0;
    if (j0 < Cs) {
        const bool whole = j0 + VEC <= Cs;
        int64_t sc[VEC];
#pragma unroll
        for (int k = 0; k < VEC; k++) sc[k] = cols ? cols[j0 + k < Cs ? j0 + k : j0] : j0 + k;
        for (int64_t i = blockIdx.y; i < Gs; i += gridDim.y) {
            const TS *srow = src + (rows ? rows[i] : i) * ld_src;
            TD *drow = dst + i * ld_dst;
            if constexpr (VEC > 1) {
                if (whole) {
                    const Vec<TS, VEC> in = *reinterpret_cast<const Vec<TS, VEC> *>(srow + j0);
                    constexpr int PER = sizeof(TD) * VEC <= 16 ? VEC : 16 / (int)sizeof(TD);      // elements per store
#pragma unroll
                    for (int c = 0; c < VEC; c += PER) {
                        Vec<TD, PER> out;
#pragma unroll
                        for (int k = 0; k < PER; k++) {
                            bad += !converts_exactly<TD, TS>(in.v[c + k]);
                            out.v[k] = convert_value<TD, TS>(in.v[c + k]);
                        }
                        *reinterpret_cast<Vec<TD, PER> *>(drow + j0 + c) = out;
                    }
                    continue;
                }
            }
#pragma unroll
            for (int k = 0; k < VEC; k++)
                if (j0 + k < Cs) {
                    const TS v = srow[sc[k]];
                    bad += !converts_exactly<TD, TS>(v);
                    drow[j0 + k] = convert_value<TD, TS>(v);
                }
        }
    }
    bad = wave_sum(bad);                                  // (every lane of the workgroup arrives here)
    if ((threadIdx.x & 63) == 0 && bad) atomicAdd(inexact, (unsigned long long)bad);
}

// What one workgroup saw of the view; the host folds the workgroups' partial results (min, max and counts: order-free).
struct RangePart {
    double lo, hi;
    int64_t ilo, ihi, non_integral, non_finite, not_f32_exact, pad;
};

template <typename TS>
__global__ __launch_bounds__(WG) void range_kernel(const TS *__restrict__ src, int64_t ld_src, const int64_t *__restrict__ rows, int64_t Gs,
                                                   const int64_t *__restrict__ cols, int64_t Cs, RangePart *parts) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    double lo = std::numeric_limits<double>::infinity(), hi = -lo;
    int64_t ilo = INT64_MAX, ihi = INT64_MIN, nint = 0, nfin = 0, n32 = 0;
    if (j < Cs) {
        const int64_t sc = cols ? cols[j] : j;
        for (int64_t i = blockIdx.y; i < Gs; i += gridDim.y) {
            const TS v = src[(rows ? rows[i] : i) * ld_src + sc];
            if constexpr (is_float_type<TS>::value) {
                const double d = (double)v;
                if (d == d) {
                    lo = d < lo ? d : lo;
                    hi = d > hi ? d : hi;
                }
                const bool finite = d - d == 0;
                nfin += !finite;
                nint += finite && (d < -9007199254740992.0 || d > 9007199254740992.0 ? false : (double)(int64_t)d != d);
                n32 += d == d && !converts_exactly<float, TS>(v);   // (a NaN narrows to a NaN: np.array_equal(..., equal_nan=True))
            } else {
                const int64_t w = (int64_t)v;
                ilo = w < ilo ? w : ilo;
                ihi = w > ihi ? w : ihi;
                n32 += !converts_exactly<float, TS>(v);
            }
        }
    }
    __shared__ RangePart sh[WG / 64];
    for (int o = 32; o > 0; o >>= 1) {
        const double l2 = __shfl_xor(lo, o), h2 = __shfl_xor(hi, o);
        const int64_t il = __shfl_xor(ilo, o), ih = __shfl_xor(ihi, o);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
        ilo = il < ilo ? il : ilo;
        ihi = ih > ihi ? ih : ihi;
        nint += __shfl_xor(nint, o);
        nfin += __shfl_xor(nfin, o);
        n32 += __shfl_xor(n32, o);
    }
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = RangePart{lo, hi, ilo, ihi, nint, nfin, n32, 0};
    __syncthreads();
    if (threadIdx.x == 0) {
        RangePart r = sh[0];
        for (int w = 1; w < (int)(blockDim.x >> 6); w++) {
            const RangePart &q = sh[w];
            r.lo = q.lo < r.lo ? q.lo : r.lo;
            r.hi = q.hi > r.hi ? q.hi : r.hi;
            r.ilo = q.ilo < r.ilo ? q.ilo : r.ilo;
            r.ihi = q.ihi > r.ihi ? q.ihi : r.ihi;
            r.non_integral += q.non_integral;
            r.non_finite += q.non_finite;
            r.not_f32_exact += q.not_f32_exact;
        }
        parts[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = r;
    }
}

size_t src_size(int dt) {
    switch (dt) {
    case CYTO_DTYPE_I64: case CYTO_DTYPE_F64: return 8;
    case CYTO_DTYPE_F32: return 4;
    case CYTO_DTYPE_U16: return 2;
    default: return 0;
    }
}
size_t dst_size(int dt) {
    switch (dt) {
    case CYTO_DTYPE_U8: return 1;
    case CYTO_DTYPE_U16: return 2;
    case CYTO_DTYPE_F32: return 4;
    case CYTO_DTYPE_I64: case CYTO_DTYPE_F64: return 8;
    default: return 0;
    }
}

#define SRC_DISPATCH(dt, ...)                                              \
    switch (dt) {                                                          \
    case CYTO_DTYPE_I64: { using TS = int64_t; __VA_ARGS__; } break;       \
    case CYTO_DTYPE_F64: { using TS = double; __VA_ARGS__; } break;        \
    case CYTO_DTYPE_U16: { using TS = uint16_t; __VA_ARGS__; } break;      \
    default: { using TS = float; __VA_ARGS__; } break;                     \
    }
#define DST_DISPATCH(dt, ...)                                              \
    switch (dt) {                                                          \
    case CYTO_DTYPE_U8: { using TD = uint8_t; __VA_ARGS__; } break;        \
    case CYTO_DTYPE_U16: { using TD = uint16_t; __VA_ARGS__; } break;      \
    case CYTO_DTYPE_I64: { using TD = int64_t; __VA_ARGS__; } break;       \
    case CYTO_DTYPE_F32: { using TD = float; __VA_ARGS__; } break;         \
    default: { using TD = double; __VA_ARGS__; } break;                    \
    }

// The arguments every entry point of a view shares; CYTO_ERR_BAD_ARG before a device is touched.
int check_view(int64_t G, int64_t C, const void *src_dev, int64_t ld_src, int src_dtype, const int64_t *rows, int64_t Gs,
               const int64_t *cols, int64_t Cs) {
    if (G < 0 || C < 0 || Gs < 0 || Cs < 0 || !src_size(src_dtype) || ld_src < C) return CYTO_ERR_BAD_ARG;
    if (!rows && Gs != G) return CYTO_ERR_BAD_ARG;
    if (!cols && Cs != C) return CYTO_ERR_BAD_ARG;
    if (Gs > 0 && Cs > 0 && !src_dev) return CYTO_ERR_BAD_ARG;
    for (int64_t i = 0; rows && i < Gs; i++)
        if (rows[i] < 0 || rows[i] >= G) return CYTO_ERR_BAD_ARG;
    for (int64_t j = 0; cols && j < Cs; j++)
        if (cols[j] < 0 || cols[j] >= C) return CYTO_ERR_BAD_ARG;
    return CYTO_OK;
}

// The position lists on the device (work buffers of the block cache, released when `s` has drained).
struct Lists {
    DevBuf rows, cols;
    int upload(const int64_t *r, int64_t Gs, const int64_t *c, int64_t Cs, hipStream_t s) {
        int rc;
        if (r) {
            if ((rc = rows.alloc((size_t)Gs * 8, s))) return rc;
            CYTO_HIP(hipMemcpyAsync(rows.p, r, (size_t)Gs * 8, hipMemcpyHostToDevice, s));
        }
        if (c) {
            if ((rc = cols.alloc((size_t)Cs * 8, s))) return rc;
            CYTO_HIP(hipMemcpyAsync(cols.p, c, (size_t)Cs * 8, hipMemcpyHostToDevice, s));
        }
        return CYTO_OK;
    }
};

template <typename TS, typename TD>
int launch_select(const void *src, int64_t ld_src, const int64_t *rows, int64_t Gs, const int64_t *cols, int64_t Cs, void *dst,
                  int64_t ld_dst, unsigned long long *inexact, hipStream_t s) {
    constexpr int VEC = 16 / (int)sizeof(TS);
    constexpr size_t OUT = sizeof(TD) * VEC <= 16 ? sizeof(TD) * VEC : 16;     // bytes of one store of the wide form
    const bool wide = !cols && Cs >= VEC && (uintptr_t)src % 16 == 0 && (size_t)ld_src * sizeof(TS) % 16 == 0 &&
                      (uintptr_t)dst % OUT == 0 && (size_t)ld_dst * sizeof(TD) % OUT == 0;
    const int64_t lanes = wide ? (Cs + VEC - 1) / VEC : Cs;
    const int wg = lanes <= 64 ? 64 : lanes <= 128 ? 128 : WG;
    const dim3 grid((unsigned)((lanes + wg - 1) / wg), (unsigned)std::min<int64_t>(Gs, MAX_ROW_BLOCKS));
    if (wide)
        hipLaunchKernelGGL((select_kernel<TS, TD, VEC>), grid, dim3(wg), 0, s, (const TS *)src, ld_src, rows, Gs, cols, Cs, (TD *)dst, ld_dst,
                           inexact);
    else
        hipLaunchKernelGGL((select_kernel<TS, TD, 1>), grid, dim3(wg), 0, s, (const TS *)src, ld_src, rows, Gs, cols, Cs, (TD *)dst, ld_dst,
                           inexact);
    CYTO_HIP(hipGetLastError());
    return CYTO_OK;
}

template <typename TS, typename TD> void check_values(const void *values, int64_t n, int8_t *ok) {
    const TS *v = static_cast<const TS *>(values);
    for (int64_t i = 0; i < n; i++) ok[i] = (int8_t)converts_exactly<TD, TS>(v[i]);
}

}  // namespace

int cyto_select(int64_t G, int64_t C, const void *src_dev, int64_t ld_src, int src_dtype, const int64_t *rows, int64_t Gs,
                const int64_t *cols, int64_t Cs, void *dst_dev, int64_t ld_dst, int dst_dtype, int64_t *inexact, int device_id,
                void *stream) {
    int rc;
    if ((rc = check_view(G, C, src_dev, ld_src, src_dtype, rows, Gs, cols, Cs))) return rc;
    if (!dst_size(dst_dtype) || ld_dst < Cs || !inexact || (Gs > 0 && Cs > 0 && !dst_dev)) return CYTO_ERR_BAD_ARG;
    if (Cs > (int64_t)0x7fffffff * 64) return CYTO_ERR_BAD_ARG;
    *inexact = 0;
    if (Gs == 0 || Cs == 0) return CYTO_OK;
    if ((rc = select_device(device_id))) return rc;
    hipStream_t s = (hipStream_t)stream;
    unsigned long long bad = 0;
    {
        DevBuf cnt;
        Lists l;
        StreamDrain drain;                                // (declared after the buffers: `s` has drained before they are released)
        drain.s = s;
        if ((rc = cnt.alloc(8, s)) || (rc = l.upload(rows, Gs, cols, Cs, s))) return rc;
        CYTO_HIP(hipMemsetAsync(cnt.p, 0, 8, s));
        SRC_DISPATCH(src_dtype, DST_DISPATCH(dst_dtype, rc = (launch_select<TS, TD>)(src_dev, ld_src, l.rows.as<int64_t>(), Gs, l.cols.as<int64_t>(),
                                                                                      Cs, dst_dev, ld_dst, cnt.as<unsigned long long>(), s)));
        if (rc) return rc;
        CYTO_HIP(hipMemcpyAsync(&bad, cnt.p, 8, hipMemcpyDeviceToHost, s));
        CYTO_HIP(hipStreamSynchronize(s));
    }
    *inexact = (int64_t)bad;
    return CYTO_OK;
}

int cyto_value_range(int64_t G, int64_t C, const void *src_dev, int64_t ld_src, int src_dtype, const int64_t *rows, int64_t Gs,
                     const int64_t *cols, int64_t Cs, double *lo, double *hi, int64_t *lo_i64, int64_t *hi_i64, int64_t *non_integral,
                     int64_t *non_finite, int64_t *not_f32_exact, int device_id, void *stream) {
    int rc;
    if ((rc = check_view(G, C, src_dev, ld_src, src_dtype, rows, Gs, cols, Cs))) return rc;
    if (!lo || !hi || !non_integral || !non_finite || !not_f32_exact) return CYTO_ERR_BAD_ARG;
    if (Cs > (int64_t)0x7fffffff * 64) return CYTO_ERR_BAD_ARG;
    RangePart r{std::numeric_limits<double>::infinity(), -std::numeric_limits<double>::infinity(), INT64_MAX, INT64_MIN, 0, 0, 0, 0};
    if (Gs > 0 && Cs > 0) {
        if ((rc = select_device(device_id))) return rc;
        hipStream_t s = (hipStream_t)stream;
        const int wg = Cs <= 64 ? 64 : Cs <= 128 ? 128 : WG;
        const dim3 grid((unsigned)((Cs + wg - 1) / wg), (unsigned)std::min<int64_t>(Gs, RANGE_ROW_BLOCKS));
        const size_t np = (size_t)grid.x * grid.y;
        std::vector<RangePart> parts(np);
        {
            DevBuf dparts;
            Lists l;
            StreamDrain drain;
            drain.s = s;
            if ((rc = dparts.alloc(np * sizeof(RangePart), s)) || (rc = l.upload(rows, Gs, cols, Cs, s))) return rc;
            SRC_DISPATCH(src_dtype, hipLaunchKernelGGL((range_kernel<TS>), grid, dim3(wg), 0, s, (const TS *)src_dev, ld_src, l.rows.as<int64_t>(),
                                                       Gs, l.cols.as<int64_t>(), Cs, dparts.as<RangePart>()));
            CYTO_HIP(hipGetLastError());
            CYTO_HIP(hipMemcpyAsync(parts.data(), dparts.p, np * sizeof(RangePart), hipMemcpyDeviceToHost, s));
            CYTO_HIP(hipStreamSynchronize(s));
        }
        for (const RangePart &q : parts) {
            r.lo = std::min(r.lo, q.lo);
            r.hi = std::max(r.hi, q.hi);
            r.ilo = std::min(r.ilo, q.ilo);
            r.ihi = std::max(r.ihi, q.ihi);
            r.non_integral += q.non_integral;
            r.non_finite += q.non_finite;
            r.not_f32_exact += q.not_f32_exact;
        }
    }
    const bool ints = src_dtype == CYTO_DTYPE_I64 || src_dtype == CYTO_DTYPE_U16;
    const bool any = Gs > 0 && Cs > 0;
    *lo = ints && any ? (double)r.ilo : r.lo;
    *hi = ints && any ? (double)r.ihi : r.hi;
    if (lo_i64) *lo_i64 = ints ? r.ilo : 0;
    if (hi_i64) *hi_i64 = ints ? r.ihi : 0;
    *non_integral = r.non_integral;
    *non_finite = r.non_finite;
    *not_f32_exact = r.not_f32_exact;
    return CYTO_OK;
}

int cyto_select_check(const void *values, int src_dtype, int64_t n, int dst_dtype, int8_t *ok) {
    if (n < 0 || !src_size(src_dtype) || !dst_size(dst_dtype) || (n > 0 && (!values || !ok))) return CYTO_ERR_BAD_ARG;
    SRC_DISPATCH(src_dtype, DST_DISPATCH(dst_dtype, (check_values<TS, TD>)(values, n, ok)));
    return CYTO_OK;
}
