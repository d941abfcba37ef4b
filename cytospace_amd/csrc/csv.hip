// csv.hip -- the place-holder expression table, <prefix>new_scRNA.csv (post_processing.write_csv_device), with its value fields
// formatted on the device: byte for byte what pandas' DataFrame.to_csv writes for the genes x selected-cells frame, or refused
// (CYTO_ERR_UNSUPPORTED) so that the caller has pandas write it.
//
// X is the G x N source matrix, cols the C source columns of the generated cells.  The file is the caller's header line, then per gene
// the caller's label bytes (quoted by the caller, with their trailing ','), the C values X[gene, cols[j]] separated by ',' and a '\n'
// (DESIGN.md 4.1d').  A gene's cells are cut into segments of 512; a field is the value's text and its terminator (',' or, for the
// gene's last cell, '\n'), 21 bytes at the most (25 with CYTO_TEXT_FRACTIONS).
//   csv_count    (a workgroup per gene and segment) the exact bytes of the segment's fields, plus the label's before segment 0; and
//                which values are outside the device grammar (a real value that is not an integer below 2^53 -- 2^24 for float32; with
//                CYTO_TEXT_FRACTIONS only a value that is not finite: every other real is written by its shortest digits, shortest.h).
//   csv_scan     (one workgroup) turns the segments' byte counts into int64 offsets into the slab's text.
//   csv_format   (a workgroup per gene and segment) computes the field lengths again, scans them, formats the fields into LDS at the
//                position their bytes have within the 16-byte chunks of the output, and stores whole chunks with 16-byte stores; the
//                partial first and last chunk go out byte by byte, and so does the label, whose length is arbitrary.
// The genes go through in slabs of whole genes: a slab's source rows are uploaded as they lie (the columns are gathered by the kernels),
// counted, scanned, formatted, downloaded into one of two pinned buffers and written; slab k + 1 runs on the other stream while slab
// k is written, so device memory is bounded by the slab, not by G.
// fmt_value is the one formatter: the count pass, the format pass and the host (cyto_csv_format_fields) all call it.
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
    static constexpr int MAX_FIELD = FRAC ? 25 : 21;     // "-9223372036854775808" and its terminator; FRAC: "-1.7976931348623157e+308"
    static constexpr int STAGE = SEG * MAX_FIELD + 16;   // a segment's fields, shifted by up to 15 bytes
};
constexpr int64_t DEFAULT_BLOCK = int64_t(32) << 20;
constexpr int64_t MAX_BLOCK = int64_t(1) << 40;

// A value as the formatter takes it.  status: 0 inside the grammar, else CYTO_CSV_ERR_* (neg and mag are then those of a zero, so
// that both passes give the value the same, short field).
// The value is mag * 10^e10; form: 0 positional, 1 scientific, 2 by the exponent, as repr(float) has it (e10 and form: FRAC only).
struct Val {
    int status;
    bool neg;
    uint64_t mag;
    int e10, form;
};

template <typename T> __host__ __device__ inline Val classify_int(T v) {
    const bool neg = v < 0;
    return Val{0, neg, neg ? (uint64_t)0 - (uint64_t)(int64_t)v : (uint64_t)v, 0, 0};
}
// pandas writes repr(float(v)): for an integer below 2^53 (a float32 is widened first: below 2^24, where the device keeps the
// window the MatrixMarket writer has) the integer's digits and ".0"; a zero keeps its sign.
// FRAC: an integer inside the window keeps the path it has without the flag; every other finite value gets its shortest digits.
// numpy writes a float32 in the scientific form when |v| < 1e-4 or |v| >= 1e16, by the value: float32(1e-4) = 0x38d1b717 lies below
// 1e-4 (its digits, 1e-04, would be positional by their exponent), and the first float32 that is no less than 1e16 is 0x5a0e1bca.
__host__ __device__ inline Val shortest(float v) {
    const uint32_t b = __builtin_bit_cast(uint32_t, v) & 0x7fffffffu;
    const Decimal d = shortest_digits32(b);
    return Val{0, false, d.digits, d.exp10, b <= 0x38d1b717u || b >= 0x5a0e1bcau ? 1 : 0};
}
__host__ __device__ inline Val shortest(double v) {
    const Decimal d = shortest_digits64(__builtin_bit_cast(uint64_t, v));
    return Val{0, false, d.digits, d.exp10, 2};
}
template <bool FRAC, typename T> __host__ __device__ inline Val classify_real(T t, double limit) {
    const double v = (double)t;
    const double a = fabs(v);
    if (!(a <= 1.7976931348623157e308)) return Val{CYTO_CSV_ERR_NONFINITE, false, 0, 0, 0};
    if (FRAC) {
        if (a < limit && a == floor(a)) return Val{0, __builtin_signbit(v) != 0, (uint64_t)a, 0, 0};
        Val r = shortest(t);
        r.neg = v < 0.0;
        return r;
    }
    if (a >= limit) return Val{CYTO_CSV_ERR_MAGNITUDE, false, 0, 0, 0};
    if (a != floor(a)) return Val{CYTO_CSV_ERR_FRACTION, false, 0, 0, 0};
    return Val{0, __builtin_signbit(v) != 0, (uint64_t)a, 0, 0};
}
template <bool FRAC> __host__ __device__ inline Val classify(uint8_t v) { return classify_int(v); }
template <bool FRAC> __host__ __device__ inline Val classify(uint16_t v) { return classify_int(v); }
template <bool FRAC> __host__ __device__ inline Val classify(int32_t v) { return classify_int(v); }
template <bool FRAC> __host__ __device__ inline Val classify(int64_t v) { return classify_int(v); }
template <bool FRAC> __host__ __device__ inline Val classify(float v) { return classify_real<FRAC>(v, 16777216.0); }
template <bool FRAC> __host__ __device__ inline Val classify(double v) { return classify_real<FRAC>(v, 9007199254740992.0); }
template <typename T> struct is_real { static constexpr bool value = false; };
template <> struct is_real<float> { static constexpr bool value = true; };
template <> struct is_real<double> { static constexpr bool value = true; };

// The value's text, without a terminator; returns its length.  WRITE = false: the length alone (o is not touched).
// FRAC, a value with e10 != 0 or form != 0 (d1 ... dnd: the digits of m, e = e10 + nd - 1 the decimal exponent of d1):
//   positional   e10 >= 0: the digits, e10 zeros, ".0"; e >= 0: a '.' after digit e + 1; e < 0: "0.", -e - 1 zeros, the digits.
//   scientific   d1[.d2 ... dnd]e[+-]XX, at least two exponent digits.
template <bool WRITE, bool FRAC> __host__ __device__ inline int fmt_value(uint8_t *o, bool real, const Val &val) {
    const bool neg = val.neg;
    const uint64_t m = val.mag;
    int n = 0;
    if (neg) {
        if (WRITE) o[n] = '-';
        n++;
    }
    const int nd = ndigits64(m);
    if (FRAC && (val.e10 != 0 || val.form != 0)) {
        const int e10 = val.e10;
        int e = e10 + nd - 1;
        if (val.form == 1 || (val.form == 2 && (e < -4 || e >= 16))) {
            if (WRITE) {
                put_digits(o + n + 1, m, nd);
                o[n] = o[n + 1];
                o[n + 1] = '.';
            }
            n += nd == 1 ? 1 : nd + 1;                  // (a lone digit: the '.' is overwritten)
            if (WRITE) {
                o[n] = 'e';
                o[n + 1] = e < 0 ? '-' : '+';
            }
            n += 2;
            if (e < 0) e = -e;
            const int ne = e < 100 ? 2 : 3;
            if (WRITE) {
                if (ne == 3) o[n] = (uint8_t)('0' + e / 100);
                o[n + ne - 2] = (uint8_t)('0' + e / 10 % 10);
                o[n + ne - 1] = (uint8_t)('0' + e % 10);
            }
            return n + ne;
        }
        if (e10 >= 0) {
            if (WRITE) {
                put_digits(o + n, m, nd);
                for (int i = 0; i < e10; i++) o[n + nd + i] = '0';
                o[n + nd + e10] = '.';
                o[n + nd + e10 + 1] = '0';
            }
            return n + nd + e10 + 2;
        }
        if (e >= 0) {
            if (WRITE) {
                put_digits(o + n + 1, m, nd);
                for (int i = 0; i <= e; i++) o[n + i] = o[n + i + 1];
                o[n + e + 1] = '.';
            }
            return n + nd + 1;
        }
        if (WRITE) {
            o[n] = '0';
            o[n + 1] = '.';
            for (int i = 0; i < -e - 1; i++) o[n + 2 + i] = '0';
            put_digits(o + n + 1 - e, m, nd);
        }
        return n + 1 - e + nd;
    }
    if (WRITE) put_digits(o + n, m, nd);
    n += nd;
    if (real) {
        if (WRITE) {
            o[n] = '.';
            o[n + 1] = '0';
        }
        n += 2;
    }
    return n;
}

// The longest field (text and terminator) a value of the type can have: what a slab's text is bounded by before it is counted.
int max_field(int dt, bool frac) {
    switch (dt) {
    case CYTO_DTYPE_U8: return 4;                        // "255,"
    case CYTO_DTYPE_U16: return 6;                       // "65535,"
    case CYTO_DTYPE_I32: return 12;                      // "-2147483648,"
    case CYTO_DTYPE_F32: return frac ? 20 : 12;          // "-16777215.0,"; "-9999999000000000.0,"
    case CYTO_DTYPE_F64: return frac ? 25 : 20;          // "-9007199254740991.0,"; "-1.7976931348623157e+308,"
    }
    return Lim<false>::MAX_FIELD;
}

// Workgroup w of the launch: the slab's gene r = w / nseg, segment s = w % nseg.  X: the slab's rows; label_off[r .. r + 1]: gene r's
// label within the file's label bytes.  seg_bytes[w] := the bytes of the segment's fields, with the label's for s = 0;
// *flags |= 1 << CYTO_CSV_ERR_* for every kind of value outside the grammar.
template <typename T, bool FRAC>
__global__ __launch_bounds__(WG) void csv_count(const T *X, int64_t ldx, const int64_t *cols, int64_t C, int nseg, const int64_t *label_off,
                                                int64_t *seg_bytes, int *flags) {
    const int64_t r = blockIdx.x / nseg;
    const int s = (int)(blockIdx.x % nseg);
    const T *xr = X + r * ldx;
    int mine = 0, bad = 0;
#pragma unroll
    for (int k = 0; k < EPT; k++) {
        const int64_t j = (int64_t)s * SEG + threadIdx.x * EPT + k;
        if (j >= C) break;
        const Val v = classify<FRAC>(xr[cols[j]]);
        if (v.status) bad |= 1 << v.status;
        mine += fmt_value<false, FRAC>(nullptr, is_real<T>::value, v) + 1;
    }
    int tot;
    wg_scan<WG>(mine, &tot);
    if (threadIdx.x == 0) seg_bytes[blockIdx.x] = tot + (s == 0 ? label_off[r + 1] - label_off[r] : 0);
    if (bad) atomicOr(flags, bad);
}

// One workgroup: seg_off[0 .. n] := exclusive prefix sum of seg_bytes (seg_off[n], also *total: the slab's bytes).
__global__ __launch_bounds__(WG) void csv_scan(const int64_t *seg_bytes, int64_t n, int64_t *seg_off, int64_t *total) {
    int64_t carry = 0;
    for (int64_t i0 = 0; i0 < n; i0 += WG) {
        const int64_t i = i0 + threadIdx.x;
        int64_t tot;
        const int64_t ex = wg_scan<WG, int64_t>(i < n ? seg_bytes[i] : 0, &tot);
        if (i < n) seg_off[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) {
        seg_off[n] = carry;
        *total = carry;
    }
}

// Workgroup w as in csv_count.  labels: the slab's label bytes, gene r's at label_off[r] - label_off[0]; out: the slab's text (16-byte
// aligned).
template <typename T, bool FRAC>
__global__ __launch_bounds__(WG) void csv_format(const T *X, int64_t ldx, const int64_t *cols, int64_t C, int nseg, const int64_t *label_off,
                                                 const uint8_t *labels, const int64_t *seg_off, uint8_t *out) {
    __shared__ uint4 stage4[(Lim<FRAC>::STAGE + 15) / 16];
    uint8_t *stage = reinterpret_cast<uint8_t *>(stage4);
    const int64_t r = blockIdx.x / nseg;
    const int s = (int)(blockIdx.x % nseg);
    const T *xr = X + r * ldx;
    Val v[EPT];
    int len[EPT], mine = 0;
#pragma unroll
    for (int k = 0; k < EPT; k++) {
        const int64_t j = (int64_t)s * SEG + threadIdx.x * EPT + k;
        len[k] = 0;
        if (j < C) {
            v[k] = classify<FRAC>(xr[cols[j]]);
            len[k] = fmt_value<false, FRAC>(nullptr, is_real<T>::value, v[k]) + 1;
        }
        mine += len[k];
    }
    int tot;
    const int ex = wg_scan<WG>(mine, &tot);
    int64_t dst = seg_off[blockIdx.x];
    if (s == 0) {                                       // the label: any length, any alignment
        const int64_t lab = label_off[r + 1] - label_off[r];
        const uint8_t *src = labels + (label_off[r] - label_off[0]);
        for (int64_t i = threadIdx.x; i < lab; i += WG) out[dst + i] = src[i];
        dst += lab;
    }
    const int shift = (int)(dst & 15);                  // stage[p] is byte (dst - shift + p) of out: chunks line up
    uint8_t *p = stage + shift + ex;
#pragma unroll
    for (int k = 0; k < EPT; k++)
        if (len[k]) {
            const int64_t j = (int64_t)s * SEG + threadIdx.x * EPT + k;
            fmt_value<true, FRAC>(p, is_real<T>::value, v[k]);
            p[len[k] - 1] = j == C - 1 ? '\n' : ',';
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
#define CSV_DISPATCH(dt, frac, ...)                                                               \
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

int cyto_csv_write(const char *path, int64_t G, int64_t N, const void *x, int64_t ldx, int x_dtype, const int64_t *cols, int64_t C,
                   const char *header, int64_t header_len, const char *labels, const int64_t *label_off, int64_t block_bytes,
                   int device_id, cyto_csv_info *info) {
    return cyto_csv_write_ex(path, G, N, x, ldx, x_dtype, cols, C, header, header_len, labels, label_off, block_bytes, device_id, 0, info);
}

int cyto_csv_write_ex(const char *path, int64_t G, int64_t N, const void *x, int64_t ldx, int x_dtype, const int64_t *cols, int64_t C,
                      const char *header, int64_t header_len, const char *labels, const int64_t *label_off, int64_t block_bytes,
                      int device_id, int flags, cyto_csv_info *info) {
    const size_t es = dtype_size(x_dtype);
    const bool frac = (flags & CYTO_TEXT_FRACTIONS) != 0;
    if (flags & ~CYTO_TEXT_FRACTIONS) return CYTO_ERR_BAD_ARG;
    if (!path || !x || !cols || !header || !labels || !label_off || !info || es == 0 || G <= 0 || N <= 0 || C <= 0 || ldx < N ||
        header_len < 0 || block_bytes < 0 || G > 0x7fffffffll || C > 0x7fffffffll)
        return CYTO_ERR_BAD_ARG;
    for (int64_t j = 0; j < C; j++)
        if (cols[j] < 0 || cols[j] >= N) return CYTO_ERR_BAD_ARG;
    if (label_off[0] < 0) return CYTO_ERR_BAD_ARG;
    for (int64_t g = 0; g < G; g++)
        if (label_off[g + 1] < label_off[g]) return CYTO_ERR_BAD_ARG;
    *info = cyto_csv_info{};
    auto refuse = [&](int kind) {                       // nothing stays at `path`, not even an earlier file
        info->reason = kind;
        unlink(path);
        return (int)CYTO_ERR_UNSUPPORTED;
    };
    int rc;
    if ((rc = select_device(device_id))) return rc;

    // (1) the slabs: whole genes whose text, at the type's longest field, fits the cap; a gene with more stands alone.  A slab's source
    // rows are capped too (N may be far above C), and so are the workgroups of one launch.
    const int nseg = (int)((C + SEG - 1) / SEG);
    const int64_t cap = std::min(block_bytes ? block_bytes : DEFAULT_BLOCK, MAX_BLOCK);
    const int64_t in_cap = 4 * cap, row_in = ldx * (int64_t)es, row_text = C * max_field(x_dtype, frac);
    const int64_t max_rows = std::max<int64_t>(1, (int64_t(1) << 30) / nseg);
    std::vector<int64_t> first;                         // slab k: genes [first[k], first[k + 1])
    int64_t most_text = 0, most_rows = 0, most_labels = 0;
    for (int64_t g = 0; g < G;) {
        int64_t e = g, text = 0;
        do {
            text += label_off[e + 1] - label_off[e] + row_text;
            e++;
        } while (e < G && e - g < max_rows && (e - g + 1) * row_in <= in_cap &&
                 text + label_off[e + 1] - label_off[e] + row_text <= cap);
        first.push_back(g);
        most_text = std::max(most_text, text);
        most_rows = std::max(most_rows, e - g);
        most_labels = std::max(most_labels, label_off[e] - label_off[g]);
        g = e;
    }
    first.push_back(G);
    const int64_t nb = (int64_t)first.size() - 1;
    info->blocks = nb;

    // (declared before the streams: they drain before any buffer or copy source / destination is freed, whatever path leaves the call)
    Mem dcols, dx[2], dseg[2], doff[2], dlab[2], dlaboff[2], scal[2], dbuf[2];
    Pinned pin;
    Events<10> ev;                                      // per buffer b, 5 * b + : upload start / end, kernels end, download start / end
    int64_t hs[2][2] = {{0, 0}, {0, 0}}, len[2] = {0, 0};
    OutFile f;
    StreamGuard st[2];
    if ((rc = st[0].acquire()) || (rc = st[1].acquire()) || (rc = ev.create()) || (rc = dcols.alloc((size_t)C * 8))) return rc;
    for (int b = 0; b < (nb > 1 ? 2 : 1); b++) {
        if ((rc = dx[b].alloc((size_t)(most_rows * row_in))) || (rc = dseg[b].alloc((size_t)(most_rows * nseg) * 8)) ||
            (rc = doff[b].alloc((size_t)(most_rows * nseg + 1) * 8)) || (rc = dlab[b].alloc((size_t)most_labels)) ||
            (rc = dlaboff[b].alloc((size_t)(most_rows + 1) * 8)) || (rc = scal[b].alloc(16)) || (rc = dbuf[b].alloc((size_t)most_text + 16)))
            return rc;
        CYTO_HIP(hipHostMalloc(&pin.p[b], (size_t)most_text + 16, hipHostMallocDefault));
    }
    f.path = path;
    f.fd = open(path, O_WRONLY | O_CREAT | O_TRUNC, 0666);
    if (f.fd < 0) return refuse(CYTO_CSV_ERR_IO);
    auto tw = std::chrono::steady_clock::now();
    if (!f.write_all(header, (size_t)header_len)) return refuse(CYTO_CSV_ERR_IO);
    info->ms_write = ms_since(tw);
    info->bytes = header_len;
    CYTO_HIP(hipMemcpyAsync(dcols.p, cols, (size_t)C * 8, hipMemcpyHostToDevice, st[0].s));
    CYTO_HIP(hipStreamSynchronize(st[0].s));            // (both streams read it)

    // (2) slab k: upload, count, scan, format -- queued without a wait: the output buffer holds the slab at its longest
    auto enqueue = [&](int64_t k) -> int {
        const int b = (int)(k & 1);
        hipStream_t s = st[b].s;
        const int64_t g0 = first[(size_t)k], R = first[(size_t)k + 1] - g0, nlab = label_off[g0 + R] - label_off[g0];
        const unsigned grid = (unsigned)(R * nseg);
        CYTO_HIP(hipEventRecord(ev[5 * b], s));
        CYTO_HIP(hipMemcpyAsync(dx[b].p, static_cast<const char *>(x) + g0 * row_in, (size_t)((R - 1) * ldx + N) * es, hipMemcpyHostToDevice, s));
        CYTO_HIP(hipMemcpyAsync(dlaboff[b].p, label_off + g0, (size_t)(R + 1) * 8, hipMemcpyHostToDevice, s));
        if (nlab > 0) CYTO_HIP(hipMemcpyAsync(dlab[b].p, labels + label_off[g0], (size_t)nlab, hipMemcpyHostToDevice, s));
        CYTO_HIP(hipMemsetAsync(scal[b].p, 0, 16, s));
        CYTO_HIP(hipEventRecord(ev[5 * b + 1], s));
        CSV_DISPATCH(x_dtype, frac, hipLaunchKernelGGL((csv_count<T, FRAC>), dim3(grid), dim3(WG), 0, s, dx[b].as<T>(), ldx, dcols.as<int64_t>(), C, nseg,
                                                 dlaboff[b].as<int64_t>(), dseg[b].as<int64_t>(), scal[b].as<int>() + 2));
        CYTO_HIP(hipGetLastError());
        hipLaunchKernelGGL(csv_scan, dim3(1), dim3(WG), 0, s, dseg[b].as<int64_t>(), R * nseg, doff[b].as<int64_t>(), scal[b].as<int64_t>());
        CYTO_HIP(hipGetLastError());
        CSV_DISPATCH(x_dtype, frac, hipLaunchKernelGGL((csv_format<T, FRAC>), dim3(grid), dim3(WG), 0, s, dx[b].as<T>(), ldx, dcols.as<int64_t>(), C, nseg,
                                                 dlaboff[b].as<int64_t>(), dlab[b].as<uint8_t>(), doff[b].as<int64_t>(),
                                                 dbuf[b].as<uint8_t>()));
        CYTO_HIP(hipGetLastError());
        CYTO_HIP(hipEventRecord(ev[5 * b + 2], s));
        CYTO_HIP(hipMemcpyAsync(hs[b], scal[b].p, 16, hipMemcpyDeviceToHost, s));
        return CYTO_OK;
    };
    // (3) slab k's kernels have run: its length and what it refuses; then its download
    auto settle = [&](int64_t k) -> int {
        const int b = (int)(k & 1);
        CYTO_HIP(hipStreamSynchronize(st[b].s));
        const int bad = (int)(hs[b][1] & 0xffffffff);
        for (int kind : {CYTO_CSV_ERR_NONFINITE, CYTO_CSV_ERR_FRACTION, CYTO_CSV_ERR_MAGNITUDE})
            if (bad & (1 << kind)) return refuse(kind);
        len[b] = hs[b][0];
        if (len[b] <= 0 || len[b] > most_text) return CYTO_ERR_INTERNAL;
        CYTO_HIP(hipEventRecord(ev[5 * b + 3], st[b].s));
        CYTO_HIP(hipMemcpyAsync(pin.p[b], dbuf[b].p, (size_t)len[b], hipMemcpyDeviceToHost, st[b].s));
        CYTO_HIP(hipEventRecord(ev[5 * b + 4], st[b].s));
        return CYTO_OK;
    };
    // (4) slab k's text has arrived: write it
    auto finish = [&](int64_t k) -> int {
        const int b = (int)(k & 1);
        CYTO_HIP(hipEventSynchronize(ev[5 * b + 4]));
        float ms = 0;
        CYTO_HIP(hipEventElapsedTime(&ms, ev[5 * b], ev[5 * b + 1]));
        info->ms_upload += ms;
        CYTO_HIP(hipEventElapsedTime(&ms, ev[5 * b + 1], ev[5 * b + 2]));
        info->ms_kernels += ms;
        CYTO_HIP(hipEventElapsedTime(&ms, ev[5 * b + 3], ev[5 * b + 4]));
        info->ms_download += ms;
        tw = std::chrono::steady_clock::now();
        if (!f.write_all(pin.p[b], (size_t)len[b])) return refuse(CYTO_CSV_ERR_IO);
        info->ms_write += ms_since(tw);
        info->bytes += len[b];
        return CYTO_OK;
    };
    if ((rc = enqueue(0))) return rc;
    for (int64_t k = 0; k < nb; k++) {
        if ((rc = settle(k))) return rc;
        if (k + 1 < nb && (rc = enqueue(k + 1))) return rc;     // (its buffers are those of slab k - 1, which has been written)
        if ((rc = finish(k))) return rc;
    }
    f.keep = true;
    return CYTO_OK;
}

int cyto_csv_format_fields(const void *values, int dtype, int64_t n, char *out, int64_t cap, int32_t *lens) {
    return cyto_csv_format_fields_ex(values, dtype, n, out, cap, lens, 0);
}

int cyto_csv_format_fields_ex(const void *values, int dtype, int64_t n, char *out, int64_t cap, int32_t *lens, int flags) {
    const bool frac = (flags & CYTO_TEXT_FRACTIONS) != 0;
    if ((flags & ~CYTO_TEXT_FRACTIONS) || n < 0 || dtype_size(dtype) == 0 || cap < (frac ? 24 : 20) * n || (n > 0 && (!values || !out || !lens)))
        return CYTO_ERR_BAD_ARG;
    uint8_t *o = reinterpret_cast<uint8_t *>(out);
    int64_t at = 0;
    for (int64_t i = 0; i < n; i++) {
        int status = 0;
        CSV_DISPATCH(dtype, frac, {
            const Val v = classify<FRAC>(static_cast<const T *>(values)[i]);
            status = v.status;
            if (!status) lens[i] = fmt_value<true, FRAC>(o + at, is_real<T>::value, v);
        });
        if (status) {
            lens[i] = -status;
            return CYTO_ERR_UNSUPPORTED;
        }
        at += lens[i];
    }
    return CYTO_OK;
}
