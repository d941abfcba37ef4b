// csv.hip -- the place-holder expression table, <prefix>new_scRNA.csv (post_processing.write_csv_device), with its value fields
// formatted on the device: byte for byte what pandas' DataFrame.to_csv writes for the genes x selected-cells frame, or refused
// (CYTO_ERR_UNSUPPORTED) so that the caller has pandas write it.
//
// X is the G x N source matrix, cols the C source columns of the generated cells.  The file is the caller's header line, then per gene
// the caller's label bytes (quoted by the caller, with their trailing ','), the C values X[gene, cols[j]] separated by ',' and a '\n'
// (DESIGN.md 4.1d').  A gene's cells are cut into segments of 512; a field is the value's text and its terminator (',' or, for the
// gene's last cell, '\n'), 21 bytes at the most.
//   csv_count    (a workgroup per gene and segment) the exact bytes of the segment's fields, plus the label's before segment 0; and
//                which values are outside the device grammar (a real value that is not an integer below 2^53 -- 2^24 for float32).
//   csv_scan     (one workgroup) turns the segments' byte counts into int64 offsets into the slab's text.
//   csv_format   (a workgroup per gene and segment) computes the field lengths again, scans them, formats the fields into LDS at the
//                position their bytes have within the 16-byte chunks of the output, and stores whole chunks with 16-byte stores; the
//                partial first and last chunk go out byte by byte, and so does the label, whose length is arbitrary.
// The genes go through in slabs of whole genes: a slab's source rows are uploaded as they lie (the columns are gathered by the kernels),
// counted, scanned, formatted, downloaded into one of two pinned buffers and written; slab k + 1 runs on the other stream while slab
// k is written, so device memory is bounded by the slab, not by G.
// fmt_value is the one formatter: the count pass, the format pass and the host (cyto_csv_format_fields) all call it.
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
constexpr int MAX_FIELD = 21;                            // "-9223372036854775808" and its terminator
constexpr int STAGE = SEG * MAX_FIELD + 16;              // a segment's fields, shifted by up to 15 bytes
constexpr int64_t DEFAULT_BLOCK = int64_t(32) << 20;
constexpr int64_t MAX_BLOCK = int64_t(1) << 40;

// A value as the formatter takes it.  status: 0 inside the grammar, else CYTO_CSV_ERR_* (neg and mag are then those of a zero, so
// that both passes give the value the same, short field).
struct Val {
    int status;
    bool neg;
    uint64_t mag;
};

template <typename T> __host__ __device__ inline Val classify_int(T v) {
    const bool neg = v < 0;
    return Val{0, neg, neg ? (uint64_t)0 - (uint64_t)(int64_t)v : (uint64_t)v};
}
// pandas writes repr(float(v)): for an integer below 2^53 (a float32 is widened first: below 2^24, where the device keeps the
// window the MatrixMarket writer has) the integer's digits and ".0"; a zero keeps its sign.
__host__ __device__ inline Val classify_real(double v, double limit) {
    const double a = fabs(v);
    if (!(a <= 1.7976931348623157e308)) return Val{CYTO_CSV_ERR_NONFINITE, false, 0};
    if (a >= limit) return Val{CYTO_CSV_ERR_MAGNITUDE, false, 0};
    if (a != floor(a)) return Val{CYTO_CSV_ERR_FRACTION, false, 0};
    return Val{0, __builtin_signbit(v) != 0, (uint64_t)a};
}
__host__ __device__ inline Val classify(uint8_t v) { return classify_int(v); }
__host__ __device__ inline Val classify(uint16_t v) { return classify_int(v); }
__host__ __device__ inline Val classify(int32_t v) { return classify_int(v); }
__host__ __device__ inline Val classify(int64_t v) { return classify_int(v); }
__host__ __device__ inline Val classify(float v) { return classify_real((double)v, 16777216.0); }
__host__ __device__ inline Val classify(double v) { return classify_real(v, 9007199254740992.0); }
template <typename T> struct is_real { static constexpr bool value = false; };
template <> struct is_real<float> { static constexpr bool value = true; };
template <> struct is_real<double> { static constexpr bool value = true; };

// The value's text, without a terminator; returns its length.  WRITE = false: the length alone (o is not touched).
template <bool WRITE> __host__ __device__ inline int fmt_value(uint8_t *o, bool real, bool neg, uint64_t m) {
    int n = 0;
    if (neg) {
        if (WRITE) o[n] = '-';
        n++;
    }
    const int nd = ndigits64(m);
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
int max_field(int dt) {
    switch (dt) {
    case CYTO_DTYPE_U8: return 4;                        // "255,"
    case CYTO_DTYPE_U16: return 6;                       // "65535,"
    case CYTO_DTYPE_I32: return 12;                      // "-2147483648,"
    case CYTO_DTYPE_F32: return 12;                      // "-16777215.0,"
    case CYTO_DTYPE_F64: return 20;                      // "-9007199254740991.0,"
    }
    return MAX_FIELD;
}

// Workgroup w of the launch: the slab's gene r = w / nseg, segment s = w % nseg.  X: the slab's rows; label_off[r .. r + 1]: gene r's
// label within the file's label bytes.  seg_bytes[w] := the bytes of the segment's fields, with the label's for s = 0;
// *flags |= 1 << CYTO_CSV_ERR_* for every kind of value outside the grammar.
template <typename T>
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
        const Val v = classify(xr[cols[j]]);
        if (v.status) bad |= 1 << v.status;
        mine += fmt_value<false>(nullptr, is_real<T>::value, v.neg, v.mag) + 1;
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
template <typename T>
__global__ __launch_bounds__(WG) void csv_format(const T *X, int64_t ldx, const int64_t *cols, int64_t C, int nseg, const int64_t *label_off,
                                                 const uint8_t *labels, const int64_t *seg_off, uint8_t *out) {
    __shared__ uint4 stage4[(STAGE + 15) / 16];
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
            v[k] = classify(xr[cols[j]]);
            len[k] = fmt_value<false>(nullptr, is_real<T>::value, v[k].neg, v[k].mag) + 1;
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
            fmt_value<true>(p, is_real<T>::value, v[k].neg, v[k].mag);
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

// CALL with T bound to the element type of CYTO_DTYPE_* dt
#define CSV_DISPATCH(dt, CALL)                                     \
    switch (dt) {                                                  \
    case CYTO_DTYPE_F32: { using T = float; CALL; } break;         \
    case CYTO_DTYPE_F64: { using T = double; CALL; } break;        \
    case CYTO_DTYPE_U16: { using T = uint16_t; CALL; } break;      \
    case CYTO_DTYPE_U8: { using T = uint8_t; CALL; } break;        \
    case CYTO_DTYPE_I32: { using T = int32_t; CALL; } break;       \
    default: { using T = int64_t; CALL; } break;                   \
    }

}  // namespace

int cyto_csv_write(const char *path, int64_t G, int64_t N, const void *x, int64_t ldx, int x_dtype, const int64_t *cols, int64_t C,
                   const char *header, int64_t header_len, const char *labels, const int64_t *label_off, int64_t block_bytes,
                   int device_id, cyto_csv_info *info) {
    const size_t es = dtype_size(x_dtype);
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
    const int64_t in_cap = 4 * cap, row_in = ldx * (int64_t)es, row_text = C * max_field(x_dtype);
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
        CSV_DISPATCH(x_dtype, hipLaunchKernelGGL(csv_count<T>, dim3(grid), dim3(WG), 0, s, dx[b].as<T>(), ldx, dcols.as<int64_t>(), C, nseg,
                                                 dlaboff[b].as<int64_t>(), dseg[b].as<int64_t>(), scal[b].as<int>() + 2));
        CYTO_HIP(hipGetLastError());
        hipLaunchKernelGGL(csv_scan, dim3(1), dim3(WG), 0, s, dseg[b].as<int64_t>(), R * nseg, doff[b].as<int64_t>(), scal[b].as<int64_t>());
        CYTO_HIP(hipGetLastError());
        CSV_DISPATCH(x_dtype, hipLaunchKernelGGL(csv_format<T>, dim3(grid), dim3(WG), 0, s, dx[b].as<T>(), ldx, dcols.as<int64_t>(), C, nseg,
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
        const int flags = (int)(hs[b][1] & 0xffffffff);
        for (int kind : {CYTO_CSV_ERR_NONFINITE, CYTO_CSV_ERR_FRACTION, CYTO_CSV_ERR_MAGNITUDE})
            if (flags & (1 << kind)) return refuse(kind);
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
    if (n < 0 || dtype_size(dtype) == 0 || cap < 20 * n || (n > 0 && (!values || !out || !lens))) return CYTO_ERR_BAD_ARG;
    uint8_t *o = reinterpret_cast<uint8_t *>(out);
    int64_t at = 0;
    for (int64_t i = 0; i < n; i++) {
        Val v{};
        bool real = false;
        CSV_DISPATCH(dtype, (v = classify(static_cast<const T *>(values)[i]), real = is_real<T>::value));
        if (v.status) {
            lens[i] = -v.status;
            return CYTO_ERR_UNSUPPORTED;
        }
        lens[i] = fmt_value<true>(o + at, real, v.neg, v.mag);
        at += lens[i];
    }
    return CYTO_OK;
}
