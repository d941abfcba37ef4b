// mtx.hip -- the assigned-expression MatrixMarket file (post_processing.write_mtx_device) formatted on the device, byte for byte what
// scipy.io.mmwrite(path, coo_matrix(X[:, cols])) writes, or refused (CYTO_ERR_UNSUPPORTED) so that the caller writes it with scipy.
//
// X is the G x N source matrix, cols the C source columns of the assigned cells.  The file is a header and one line
// "<gene+1> <cell+1> <value>\n" per non-zero X[gene, cols[cell]], genes ascending, then cells ascending.
//   mtx_count    (a workgroup per gene) walks the gene's cells a segment of 512 at a time: the non-zeros and the exact bytes of their
//                lines per segment, the segment's offset within the gene's text, the gene's totals; and which values are outside the
//                device grammar (a real value that is not an integer below 2^53 -- 2^24 for float32; with CYTO_TEXT_FRACTIONS only a
//                value that is not finite: every other real is written by its shortest digits, shortest.h).
//   mtx_scan     (one workgroup) turns the genes' byte counts into int64 offsets into the body, and sums the non-zeros.
//   mtx_format   (a workgroup per gene and segment) computes the line lengths again, scans them, formats the lines into LDS at the
//                position their bytes have within the 16-byte chunks of the output, and stores whole chunks with 16-byte stores;
//                the partial first and last chunk go out byte by byte.
// The body is formatted in blocks of whole genes that fit a bounded device buffer; block k is downloaded into one of two pinned
// buffers while block k + 1 is formatted and block k - 1 is written to the file.
// fmt_line is the one formatter: the count pass, the format pass and the host (cyto_mtx_format_entries) all call it.
// FRAC: the instantiations of CYTO_TEXT_FRACTIONS (real types only); without it everything is as it was before the flag existed.
#include "shortest.h"
#include "text_write.h"

#include <fcntl.h>
#include <math.h>

#include <algorithm>
#include <vector>

namespace {

using namespace cyto;

constexpr int WG = 256;
constexpr int EPT = 2;                                   // consecutive cells per thread
constexpr int SEG = WG * EPT;                            // cells per segment
template <bool FRAC> struct Lim {
    static constexpr int MAX_VALUE = FRAC ? 24 : 21;     // "-9.007199254740991E15", an int64 takes at most 20; FRAC: "-1.7976931348623157E-308"
    static constexpr int MAX_LINE = 10 + 1 + 10 + 1 + MAX_VALUE + 1;   // G and C are below 2^31: at most 10 digits each
    static constexpr int STAGE = SEG * MAX_LINE + 16;    // a segment's text, shifted by up to 15 bytes
};
constexpr int64_t DEFAULT_BLOCK = int64_t(32) << 20;

// A value as the formatter takes it.  status: 0 a non-zero inside the grammar, 1 a zero (not written), else CYTO_MTX_ERR_*.
// The value is mag * 10^e10 (e10 != 0 only with FRAC).
struct Val {
    int status;
    bool neg;
    uint64_t mag;
    int e10;
};

template <typename T> __host__ __device__ inline Val classify_int(T v) {
    const bool neg = v < 0;
    const uint64_t m = neg ? (uint64_t)0 - (uint64_t)(int64_t)v : (uint64_t)v;
    return Val{m == 0 ? 1 : 0, neg, m, 0};
}
__host__ __device__ inline Decimal shortest(float v) { return shortest_digits32(__builtin_bit_cast(uint32_t, v)); }
__host__ __device__ inline Decimal shortest(double v) { return shortest_digits64(__builtin_bit_cast(uint64_t, v)); }
// FRAC: an integer inside the window keeps the path it has without the flag; every other finite value gets its shortest digits.
template <bool FRAC, typename T> __host__ __device__ inline Val classify_real(T v, double limit) {
    const double w = (double)v;
    if (w == 0.0) return Val{1, false, 0, 0};
    const double a = fabs(w);
    if (!(a <= 1.7976931348623157e308)) return Val{CYTO_MTX_ERR_NONFINITE, false, 0, 0};
    if (FRAC) {
        if (a < limit && a == floor(a)) return Val{0, w < 0.0, (uint64_t)a, 0};
        const Decimal d = shortest(v);
        return Val{0, w < 0.0, d.digits, d.exp10};
    }
    if (a >= limit) return Val{CYTO_MTX_ERR_MAGNITUDE, false, 0, 0};
    if (a != floor(a)) return Val{CYTO_MTX_ERR_FRACTION, false, 0, 0};
    return Val{0, w < 0.0, (uint64_t)a, 0};
}
template <bool FRAC> __host__ __device__ inline Val classify(uint8_t v) { return classify_int(v); }
template <bool FRAC> __host__ __device__ inline Val classify(uint16_t v) { return classify_int(v); }
template <bool FRAC> __host__ __device__ inline Val classify(int32_t v) { return classify_int(v); }
template <bool FRAC> __host__ __device__ inline Val classify(int64_t v) { return classify_int(v); }
// scipy writes the shortest digits that read back as the same value OF THE SOURCE TYPE: they are the integer's own digits while
// the type's spacing is at most 1, that is below 2^24 for float32 and below 2^53 for float64.
template <bool FRAC> __host__ __device__ inline Val classify(float v) { return classify_real<FRAC>(v, 16777216.0); }
template <bool FRAC> __host__ __device__ inline Val classify(double v) { return classify_real<FRAC>(v, 9007199254740992.0); }
template <typename T> struct is_real { static constexpr bool value = false; };
template <> struct is_real<float> { static constexpr bool value = true; };
template <> struct is_real<double> { static constexpr bool value = true; };

// The value's text; returns its length.  WRITE = false: the length alone (o is not touched).
// integer field: plain decimal.  real field: the digits of m without trailing zeros, a '.' after the first when more than one is
// left, and "E<k>", k = the digit count of m minus 1 plus e10 (the decimal exponent of the first digit), when k != 0.
template <bool WRITE, bool FRAC> __host__ __device__ inline int fmt_value(uint8_t *o, bool real, bool neg, uint64_t m, int e10) {
    int n = 0;
    if (neg) {
        if (WRITE) o[n] = '-';
        n++;
    }
    const int nd = ndigits64(m);
    if (!real) {
        if (WRITE) put_digits(o + n, m, nd);
        return n + nd;
    }
    int sig = nd;
    if (m <= 0xffffffffull) {
        uint32_t s = (uint32_t)m;
        while (s % 10u == 0) s /= 10u, sig--;
        m = s;
    } else {
        while (m % 10u == 0) m /= 10u, sig--;
    }
    if (sig == 1) {
        if (WRITE) o[n] = (uint8_t)('0' + m);
        n++;
    } else {
        if (WRITE) {
            put_digits(o + n + 1, m, sig);
            o[n] = o[n + 1];
            o[n + 1] = '.';
        }
        n += sig + 1;
    }
    if (FRAC) {                                         // -324 <= k <= 308: no '+', no padding
        int k = nd - 1 + e10;
        if (k != 0) {
            if (WRITE) o[n] = 'E';
            n++;
            if (k < 0) {
                if (WRITE) o[n] = '-';
                n++;
                k = -k;
            }
            const int ne = ndigits32((uint32_t)k);
            if (WRITE) put_digits(o + n, (uint64_t)k, ne);
            n += ne;
        }
        return n;
    }
    int k = nd - 1;                                      // at most 15
    if (k > 0) {
        if (WRITE) o[n] = 'E';
        n++;
        if (k >= 10) {
            if (WRITE) o[n] = '1';
            n++;
            k -= 10;
        }
        if (WRITE) o[n] = (uint8_t)('0' + k);
        n++;
    }
    return n;
}

// "<row1> <col1> <value>\n"; returns its length.
template <bool WRITE, bool FRAC> __host__ __device__ inline int fmt_line(uint8_t *o, uint64_t row1, uint64_t col1, bool real, const Val &v) {
    const int nr = ndigits64(row1), nc = ndigits64(col1);
    if (WRITE) {
        put_digits(o, row1, nr);
        o[nr] = ' ';
        put_digits(o + nr + 1, col1, nc);
        o[nr + 1 + nc] = ' ';
    }
    int n = nr + nc + 2;
    n += fmt_value<WRITE, FRAC>(o + n, real, v.neg, v.mag, v.e10);
    if (WRITE) o[n] = '\n';
    return n + 1;
}

// A workgroup per gene g.  seg_off[g * nseg + s] := the bytes of gene g's lines before segment s; row_bytes[g], row_nnz[g] := its
// totals; *flags |= 1 << CYTO_MTX_ERR_* for every kind of value outside the grammar.
template <typename T, bool FRAC>
__global__ __launch_bounds__(WG) void mtx_count(const T *X, int64_t ldx, const int64_t *cols, int64_t C, int nseg, int64_t *seg_off,
                                                int64_t *row_bytes, int64_t *row_nnz, int *flags) {
    const int64_t g = blockIdx.x;
    const T *xr = X + g * ldx;
    int64_t run = 0, nz = 0;
    int bad = 0;
    for (int s = 0; s < nseg; s++) {
        int packed = 0;                                 // bytes (at most SEG * MAX_LINE < 2^16) | non-zeros << 16
#pragma unroll
        for (int k = 0; k < EPT; k++) {
            const int64_t j = (int64_t)s * SEG + threadIdx.x * EPT + k;
            if (j >= C) break;
            const Val v = classify<FRAC>(xr[cols[j]]);
            if (v.status == 0) packed += (1 << 16) + fmt_line<false, FRAC>(nullptr, (uint64_t)g + 1, (uint64_t)j + 1, is_real<T>::value, v);
            else if (v.status > 1) bad |= 1 << v.status;
        }
        int tot;
        wg_scan<WG>(packed, &tot);
        if (threadIdx.x == 0) seg_off[g * nseg + s] = run;
        run += tot & 0xffff;
        nz += tot >> 16;
    }
    if (threadIdx.x == 0) {
        row_bytes[g] = run;
        row_nnz[g] = nz;
    }
    if (bad) atomicOr(flags, bad);
}

// One workgroup: row_off[0 .. G] := exclusive prefix sum of row_bytes (row_off[G]: the body's bytes), *nnz := the sum of row_nnz.
__global__ __launch_bounds__(WG) void mtx_scan(const int64_t *row_bytes, const int64_t *row_nnz, int64_t G, int64_t *row_off, int64_t *nnz) {
    int64_t carry = 0, nz = 0;
    for (int64_t g0 = 0; g0 < G; g0 += WG) {
        const int64_t g = g0 + threadIdx.x;
        int64_t tot, tnz;
        const int64_t ex = wg_scan<WG, int64_t>(g < G ? row_bytes[g] : 0, &tot);
        wg_scan<WG, int64_t>(g < G ? row_nnz[g] : 0, &tnz);
        if (g < G) row_off[g] = carry + ex;
        carry += tot;
        nz += tnz;
    }
    if (threadIdx.x == 0) {
        row_off[G] = carry;
        *nnz = nz;
    }
}

// Workgroup w of the launch: gene g0 + w / nseg, segment w % nseg.  out: the block's text, its first byte being byte `base` of the body
// (out is 16-byte aligned).
template <typename T, bool FRAC>
__global__ __launch_bounds__(WG) void mtx_format(const T *X, int64_t ldx, const int64_t *cols, int64_t C, int nseg, int64_t g0,
                                                 const int64_t *row_off, const int64_t *seg_off, int64_t base, uint8_t *out) {
    __shared__ uint4 stage4[(Lim<FRAC>::STAGE + 15) / 16];
    uint8_t *stage = reinterpret_cast<uint8_t *>(stage4);
    const int64_t g = g0 + blockIdx.x / nseg;
    const int s = (int)(blockIdx.x % nseg);
    const T *xr = X + g * ldx;
    Val v[EPT];
    int len[EPT], mine = 0;
#pragma unroll
    for (int k = 0; k < EPT; k++) {
        const int64_t j = (int64_t)s * SEG + threadIdx.x * EPT + k;
        len[k] = 0;
        if (j < C) {
            v[k] = classify<FRAC>(xr[cols[j]]);
            if (v[k].status == 0) len[k] = fmt_line<false, FRAC>(nullptr, (uint64_t)g + 1, (uint64_t)j + 1, is_real<T>::value, v[k]);
        }
        mine += len[k];
    }
    int tot;
    const int ex = wg_scan<WG>(mine, &tot);
    if (tot == 0) return;
    const int64_t dst = row_off[g] - base + seg_off[g * nseg + s];
    const int shift = (int)(dst & 15);                  // stage[p] is byte (dst - shift + p) of out: chunks line up
    uint8_t *p = stage + shift + ex;
#pragma unroll
    for (int k = 0; k < EPT; k++)
        if (len[k]) {
            const int64_t j = (int64_t)s * SEG + threadIdx.x * EPT + k;
            fmt_line<true, FRAC>(p, (uint64_t)g + 1, (uint64_t)j + 1, is_real<T>::value, v[k]);
            p += len[k];
        }
    __syncthreads();
    uint8_t *o = out + (dst - shift);
    const int span = shift + tot;
    for (int c = threadIdx.x; c * 16 < span; c += WG) {
        const int lo = c * 16, hi = lo + 16;
        if (lo >= shift && hi <= span) {
            *reinterpret_cast<uint4 *>(o + lo) = stage4[c];
        } else {
            for (int b = lo < shift ? shift : lo; b < (hi < span ? hi : span); b++) o[b] = stage[b];
        }
    }
}

// The statement(s) after frac, with T bound to the element type of CYTO_DTYPE_* dt and FRAC to frac (false for the integer types, whose
// text has one form)
#define MTX_DISPATCH(dt, frac, ...)                                                               \
    switch (dt) {                                                                                 \
    case CYTO_DTYPE_F32:                                                                          \
        if (frac) { using T = float; constexpr bool FRAC = true; __VA_ARGS__; }                   \
        else { using T = float; constexpr bool FRAC = false; __VA_ARGS__; }                       \
        break;                                                                                    \
    case CYTO_DTYPE_F64:                                                                          \
        if (frac) { using T = double; constexpr bool FRAC = true; __VA_ARGS__; }                  \
        else { using T = double; constexpr bool FRAC = false; __VA_ARGS__; }                      \
        break;                                                                                    \
    case CYTO_DTYPE_U16: { using T = uint16_t; constexpr bool FRAC = false; __VA_ARGS__; } break; \
    case CYTO_DTYPE_U8: { using T = uint8_t; constexpr bool FRAC = false; __VA_ARGS__; } break;   \
    case CYTO_DTYPE_I32: { using T = int32_t; constexpr bool FRAC = false; __VA_ARGS__; } break;  \
    default: { using T = int64_t; constexpr bool FRAC = false; __VA_ARGS__; } break;              \
    }

}  // namespace

int cyto_mtx_write(const char *path, int64_t G, int64_t N, const void *x, int64_t ldx, int x_dtype, const int64_t *cols, int64_t C,
                   int64_t block_bytes, int device_id, cyto_mtx_info *info) {
    return cyto_mtx_write_ex(path, G, N, x, ldx, x_dtype, cols, C, block_bytes, device_id, 0, info);
}

namespace {
// cyto_mtx_write_ex (on_device = false: x is a host matrix, uploaded whole) and cyto_mtx_write_dev (true: the kernels read x where it lies)
int mtx_write_impl(const char *path, int64_t G, int64_t N, const void *x, int64_t ldx, int x_dtype, const int64_t *cols, int64_t C,
                   int64_t block_bytes, int device_id, int flags, cyto_mtx_info *info, bool on_device) {
    const size_t es = dtype_size(x_dtype);
    const bool frac = (flags & CYTO_TEXT_FRACTIONS) != 0;
    if ((flags & ~CYTO_TEXT_FRACTIONS) || !path || !x || !cols || !info || es == 0 || G <= 0 || N <= 0 || C <= 0 || ldx < N || block_bytes < 0 || G > 0x7fffffffll ||
        C > 0x7fffffffll)
        return CYTO_ERR_BAD_ARG;
    for (int64_t j = 0; j < C; j++)
        if (cols[j] < 0 || cols[j] >= N) return CYTO_ERR_BAD_ARG;
    *info = cyto_mtx_info{};
    const bool real = x_dtype == CYTO_DTYPE_F32 || x_dtype == CYTO_DTYPE_F64;
    info->field = real ? 1 : 0;
    auto refuse = [&](int kind) {                       // nothing stays at `path`, not even an earlier file
        info->reason = kind;
        unlink(path);
        return (int)CYTO_ERR_UNSUPPORTED;
    };
    if (G == C) return refuse(CYTO_MTX_ERR_SQUARE);     // scipy looks for symmetry in a square matrix and may write a triangle
    int rc;
    if ((rc = select_device(device_id))) return rc;
    const int nseg = (int)((C + SEG - 1) / SEG);
    // (declared before the streams: they drain before any buffer or copy source / destination is freed, whatever path leaves the call)
    Mem dx, dcols, seg_off, row_bytes, row_nnz, row_off, scal, dbuf[2];
    Pinned pin;
    Events<8> ev;                                       // per buffer b: format start / end (b, 2 + b), download start / end (4 + b, 6 + b)
    std::vector<int64_t> hoff((size_t)G + 1);
    int64_t hs[2] = {0, 0};
    OutFile f;
    StreamGuard sg, sc;
    if ((rc = sg.acquire()) || (rc = sc.acquire()) || (rc = ev.create())) return rc;
    if ((!on_device && (rc = dx.alloc((size_t)(G * ldx) * es))) || (rc = dcols.alloc((size_t)C * 8)) || (rc = seg_off.alloc((size_t)(G * nseg) * 8)) ||
        (rc = row_bytes.alloc((size_t)G * 8)) || (rc = row_nnz.alloc((size_t)G * 8)) || (rc = row_off.alloc((size_t)(G + 1) * 8)) ||
        (rc = scal.alloc(16)))
        return rc;

    // (1) the matrix and the column list
    const auto t0 = std::chrono::steady_clock::now();
    if (!on_device) CYTO_HIP(hipMemcpyAsync(dx.p, x, (size_t)(G * ldx) * es, hipMemcpyHostToDevice, sg.s));
    const void *xp = on_device ? x : dx.p;              // the matrix as the kernels see it
    CYTO_HIP(hipMemcpyAsync(dcols.p, cols, (size_t)C * 8, hipMemcpyHostToDevice, sg.s));
    CYTO_HIP(hipStreamSynchronize(sg.s));
    info->ms_upload = ms_since(t0);

    // (2) counts, offsets, the values outside the grammar
    const auto t1 = std::chrono::steady_clock::now();
    CYTO_HIP(hipMemsetAsync(scal.p, 0, 16, sg.s));
    MTX_DISPATCH(x_dtype, frac, hipLaunchKernelGGL((mtx_count<T, FRAC>), dim3((unsigned)G), dim3(WG), 0, sg.s, (const T *)xp, ldx, dcols.as<int64_t>(), C,
                                             nseg, seg_off.as<int64_t>(), row_bytes.as<int64_t>(), row_nnz.as<int64_t>(),
                                             scal.as<int>() + 2));
    CYTO_HIP(hipGetLastError());
    hipLaunchKernelGGL(mtx_scan, dim3(1), dim3(WG), 0, sg.s, row_bytes.as<int64_t>(), row_nnz.as<int64_t>(), G, row_off.as<int64_t>(),
                       scal.as<int64_t>());
    CYTO_HIP(hipGetLastError());
    CYTO_HIP(hipMemcpyAsync(hs, scal.p, 16, hipMemcpyDeviceToHost, sg.s));
    CYTO_HIP(hipMemcpyAsync(hoff.data(), row_off.p, (size_t)(G + 1) * 8, hipMemcpyDeviceToHost, sg.s));
    CYTO_HIP(hipStreamSynchronize(sg.s));
    info->ms_kernels = ms_since(t1);
    const int bad = (int)(hs[1] & 0xffffffff);
    for (int kind : {CYTO_MTX_ERR_NONFINITE, CYTO_MTX_ERR_FRACTION, CYTO_MTX_ERR_MAGNITUDE})
        if (bad & (1 << kind)) return refuse(kind);
    const int64_t body = hoff[(size_t)G];
    info->nnz = hs[0];

    // (3) the header; the body in blocks of whole genes
    char head[128];
    if (hs[0] == 0) info->field = 1;                    // scipy names the field of a matrix without entries "real", whatever its type
    const int nh = snprintf(head, sizeof head, "%%%%MatrixMarket matrix coordinate %s general\n%%\n%lld %lld %lld\n",
                            info->field ? "real" : "integer", (long long)G, (long long)C, (long long)hs[0]);
    info->bytes = nh + body;
    f.path = path;
    f.fd = open(path, O_WRONLY | O_CREAT | O_TRUNC, 0666);
    if (f.fd < 0) return refuse(CYTO_MTX_ERR_IO);
    auto io_failed = [&]() { return refuse(CYTO_MTX_ERR_IO); };
    auto tw = std::chrono::steady_clock::now();
    if (!f.write_all(head, (size_t)nh)) return io_failed();
    info->ms_write = ms_since(tw);
    if (body == 0) {
        f.keep = true;
        return CYTO_OK;
    }
    const int64_t cap = block_bytes ? block_bytes : DEFAULT_BLOCK;
    std::vector<int64_t> first;                         // block k: genes [first[k], first[k + 1]); a gene larger than the cap stands alone
    int64_t largest = 0;
    for (int64_t g = 0; g < G;) {
        int64_t e = g + 1;
        while (e < G && hoff[(size_t)e + 1] - hoff[(size_t)g] <= cap) e++;
        first.push_back(g);
        largest = std::max(largest, hoff[(size_t)e] - hoff[(size_t)g]);
        g = e;
    }
    first.push_back(G);
    const int64_t nb = (int64_t)first.size() - 1;
    info->blocks = nb;
    const size_t bufsz = (size_t)largest + 16;
    for (int b = 0; b < (nb > 1 ? 2 : 1); b++) {
        if ((rc = dbuf[b].alloc(bufsz))) return rc;
        CYTO_HIP(hipHostMalloc(&pin.p[b], bufsz, hipHostMallocDefault));
    }
    const int64_t max_rows = std::max<int64_t>(1, (int64_t(1) << 30) / nseg);      // workgroups of one launch
    auto block_len = [&](int64_t k) { return hoff[(size_t)first[(size_t)k + 1]] - hoff[(size_t)first[(size_t)k]]; };
    auto finish = [&](int64_t k) -> int {               // block k has been formatted and its download queued: wait, write
        const int b = (int)(k & 1);
        const int64_t n = block_len(k);
        if (n == 0) return CYTO_OK;
        CYTO_HIP(hipEventSynchronize(ev[6 + b]));
        float ms = 0;
        CYTO_HIP(hipEventElapsedTime(&ms, ev[b], ev[2 + b]));
        info->ms_kernels += ms;
        CYTO_HIP(hipEventElapsedTime(&ms, ev[4 + b], ev[6 + b]));
        info->ms_download += ms;
        tw = std::chrono::steady_clock::now();
        if (!f.write_all(pin.p[b], (size_t)n)) return io_failed();
        info->ms_write += ms_since(tw);
        return CYTO_OK;
    };
    for (int64_t k = 0; k < nb; k++) {
        const int b = (int)(k & 1);
        const int64_t ga = first[(size_t)k], gb = first[(size_t)k + 1], n = block_len(k);
        if (n > 0) {
            CYTO_HIP(hipEventRecord(ev[b], sg.s));
            for (int64_t r0 = ga; r0 < gb; r0 += max_rows) {
                const int64_t rows = std::min(max_rows, gb - r0);
                MTX_DISPATCH(x_dtype, frac, hipLaunchKernelGGL((mtx_format<T, FRAC>), dim3((unsigned)(rows * nseg)), dim3(WG), 0, sg.s, (const T *)xp, ldx,
                                                         dcols.as<int64_t>(), C, nseg, r0, row_off.as<int64_t>(), seg_off.as<int64_t>(),
                                                         hoff[(size_t)ga], dbuf[b].as<uint8_t>()));
                CYTO_HIP(hipGetLastError());
            }
            CYTO_HIP(hipEventRecord(ev[2 + b], sg.s));
            CYTO_HIP(hipStreamWaitEvent(sc.s, ev[2 + b], 0));
            CYTO_HIP(hipEventRecord(ev[4 + b], sc.s));
            CYTO_HIP(hipMemcpyAsync(pin.p[b], dbuf[b].p, (size_t)n, hipMemcpyDeviceToHost, sc.s));
            CYTO_HIP(hipEventRecord(ev[6 + b], sc.s));
        }
        if (k > 0 && (rc = finish(k - 1))) return rc;
    }
    if ((rc = finish(nb - 1))) return rc;
    f.keep = true;
    return CYTO_OK;
}
}  // namespace

int cyto_mtx_write_ex(const char *path, int64_t G, int64_t N, const void *x, int64_t ldx, int x_dtype, const int64_t *cols, int64_t C,
                      int64_t block_bytes, int device_id, int flags, cyto_mtx_info *info) {
    return mtx_write_impl(path, G, N, x, ldx, x_dtype, cols, C, block_bytes, device_id, flags, info, false);
}

int cyto_mtx_write_dev(const char *path, int64_t G, int64_t N, const void *x_dev, int64_t ldx, int x_dtype, const int64_t *cols, int64_t C,
                       int64_t block_bytes, int device_id, int flags, cyto_mtx_info *info) {
    return mtx_write_impl(path, G, N, x_dev, ldx, x_dtype, cols, C, block_bytes, device_id, flags, info, true);
}

int cyto_mtx_format_entries(const int64_t *rows, const int64_t *cols, const void *values, int dtype, int64_t n, char *out,
                            int64_t *offsets) {
    return cyto_mtx_format_entries_ex(rows, cols, values, dtype, n, out, offsets, 0);
}

int cyto_mtx_format_entries_ex(const int64_t *rows, const int64_t *cols, const void *values, int dtype, int64_t n, char *out,
                               int64_t *offsets, int flags) {
    if ((flags & ~CYTO_TEXT_FRACTIONS) || n < 0 || !offsets || dtype_size(dtype) == 0 || (n > 0 && (!rows || !cols || !values || !out)))
        return CYTO_ERR_BAD_ARG;
    const bool frac = (flags & CYTO_TEXT_FRACTIONS) != 0;
    uint8_t *o = reinterpret_cast<uint8_t *>(out);
    int64_t at = 0;
    offsets[0] = 0;
    for (int64_t i = 0; i < n; i++) {
        if (rows[i] < 0 || cols[i] < 0) return CYTO_ERR_BAD_ARG;
        int len = 0, status = 0;
        MTX_DISPATCH(dtype, frac, {
            const Val v = classify<FRAC>(static_cast<const T *>(values)[i]);
            status = v.status;
            if (status == 0) len = fmt_line<true, FRAC>(o + at, (uint64_t)rows[i] + 1, (uint64_t)cols[i] + 1, is_real<T>::value, v);
        });
        if (status > 1) return CYTO_ERR_UNSUPPORTED;
        at += len;
        offsets[i + 1] = at;
    }
    return CYTO_OK;
}

int cyto_shortest_digits(const void *values, int dtype, int64_t n, uint64_t *digits, int32_t *exp10) {
    if (n < 0 || (dtype != CYTO_DTYPE_F32 && dtype != CYTO_DTYPE_F64) || (n > 0 && (!values || !digits || !exp10))) return CYTO_ERR_BAD_ARG;
    for (int64_t i = 0; i < n; i++) {
        Decimal d{0, 0};
        if (dtype == CYTO_DTYPE_F32) {
            const uint32_t b = static_cast<const uint32_t *>(values)[i] & 0x7fffffffu;
            if (b >= 0x7f800000u) return CYTO_ERR_BAD_ARG;
            if (b) d = shortest_digits32(b);
        } else {
            const uint64_t b = static_cast<const uint64_t *>(values)[i] & 0x7fffffffffffffffull;
            if (b >= 0x7ff0000000000000ull) return CYTO_ERR_BAD_ARG;
            if (b) d = shortest_digits64(b);
        }
        digits[i] = d.digits;
        exp10[i] = d.exp10;
    }
    return CYTO_OK;
}

int cyto_text_pow10(int k, uint64_t out[2]) {
    if (!out || k < POW10_MIN || k > POW10_MAX) return CYTO_ERR_BAD_ARG;
    const Pow10 g = pow10_entry(k);
    out[0] = g.hi;
    out[1] = g.lo;
    return CYTO_OK;
}
