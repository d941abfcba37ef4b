// table.hip -- a dense delimited text table (common.py:read_file_device) parsed on the device, value for value what
// pd.read_csv(path, sep, header=0, index_col=0) gives, or refused (CYTO_ERR_UNSUPPORTED) so that the caller reads it with pandas.
//
// The caller parses the header line (pandas does) and passes where the data lines start and how many data columns they have.
//   upload       the file is read in chunks into two pinned buffers; each chunk is uploaded while the next one is read.
//   tbl_lines    (a workgroup per 64 KiB) counts the '\n' of the data region and checks its bytes: no '"', no control byte but the
//                delimiter, '\r' and '\n', and '\r' only before '\n'.  tbl_scan_blocks turns the block counts into offsets, and
//                tbl_lines<true> writes the position of every '\n': the line ends.
//   tbl_fields   (a workgroup per line; a thread per 16-byte slice, 4 KiB per round) counts the delimiters of its slice and scans
//                the counts across the workgroup: every delimiter knows the column of the token after it, which the thread parses.
//                Pass 1 checks the field count and every token and sets the per-column "has a decimal token" flags; pass 2
//                writes every value in its column's final type (int64 or float64 bits) into the G x C row-major result.
//   tbl_labels   packs the row labels (field 0), one per line, for pandas to infer the index from.
#include "text_scan.h"

#include <fcntl.h>
#include <math.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <memory>
#include <new>
#include <vector>

namespace {

using namespace cyto;

#define CYTO_P10_LIST                                                                                                         \
    1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15,                                    \
    1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22, 1e23, 1e24, 1e25, 1e26, 1e27, 1e28, 1e29, 1e30, 1e31,                          \
    1e32, 1e33, 1e34, 1e35, 1e36, 1e37, 1e38, 1e39, 1e40, 1e41, 1e42, 1e43, 1e44, 1e45, 1e46, 1e47,                          \
    1e48, 1e49, 1e50, 1e51, 1e52, 1e53, 1e54, 1e55, 1e56, 1e57, 1e58, 1e59, 1e60, 1e61, 1e62, 1e63,                          \
    1e64, 1e65, 1e66, 1e67, 1e68, 1e69, 1e70, 1e71, 1e72, 1e73, 1e74, 1e75, 1e76, 1e77, 1e78, 1e79,                          \
    1e80, 1e81, 1e82, 1e83, 1e84, 1e85, 1e86, 1e87, 1e88, 1e89, 1e90, 1e91, 1e92, 1e93, 1e94, 1e95,                          \
    1e96, 1e97, 1e98, 1e99, 1e100, 1e101, 1e102, 1e103, 1e104, 1e105, 1e106, 1e107, 1e108, 1e109, 1e110, 1e111,              \
    1e112, 1e113, 1e114, 1e115, 1e116, 1e117, 1e118, 1e119, 1e120, 1e121, 1e122, 1e123, 1e124, 1e125, 1e126, 1e127,          \
    1e128, 1e129, 1e130, 1e131, 1e132, 1e133, 1e134, 1e135, 1e136, 1e137, 1e138, 1e139, 1e140, 1e141, 1e142, 1e143,          \
    1e144, 1e145, 1e146, 1e147, 1e148, 1e149, 1e150, 1e151, 1e152, 1e153, 1e154, 1e155, 1e156, 1e157, 1e158, 1e159,          \
    1e160, 1e161, 1e162, 1e163, 1e164, 1e165, 1e166, 1e167, 1e168, 1e169, 1e170, 1e171, 1e172, 1e173, 1e174, 1e175,          \
    1e176, 1e177, 1e178, 1e179, 1e180, 1e181, 1e182, 1e183, 1e184, 1e185, 1e186, 1e187, 1e188, 1e189, 1e190, 1e191,          \
    1e192, 1e193, 1e194, 1e195, 1e196, 1e197, 1e198, 1e199, 1e200, 1e201, 1e202, 1e203, 1e204, 1e205, 1e206, 1e207,          \
    1e208, 1e209, 1e210, 1e211, 1e212, 1e213, 1e214, 1e215, 1e216, 1e217, 1e218, 1e219, 1e220, 1e221, 1e222, 1e223,          \
    1e224, 1e225, 1e226, 1e227, 1e228, 1e229, 1e230, 1e231, 1e232, 1e233, 1e234, 1e235, 1e236, 1e237, 1e238, 1e239,          \
    1e240, 1e241, 1e242, 1e243, 1e244, 1e245, 1e246, 1e247, 1e248, 1e249, 1e250, 1e251, 1e252, 1e253, 1e254, 1e255,          \
    1e256, 1e257, 1e258, 1e259, 1e260, 1e261, 1e262, 1e263, 1e264, 1e265, 1e266, 1e267, 1e268, 1e269, 1e270, 1e271,          \
    1e272, 1e273, 1e274, 1e275, 1e276, 1e277, 1e278, 1e279, 1e280, 1e281, 1e282, 1e283, 1e284, 1e285, 1e286, 1e287,          \
    1e288, 1e289, 1e290, 1e291, 1e292, 1e293, 1e294, 1e295, 1e296, 1e297, 1e298, 1e299, 1e300, 1e301, 1e302, 1e303,          \
    1e304, 1e305, 1e306, 1e307, 1e308

// (each side of the compilation uses one of the two)
[[maybe_unused]] __constant__ double P10_DEV[309] = {CYTO_P10_LIST};
[[maybe_unused]] const double P10_HOST[309] = {CYTO_P10_LIST};

enum { TOK_INT = 0, TOK_DEC = 1, TOK_BAD = 2, TOK_RANGE = 3 };

__host__ __device__ inline bool is_digit(uint8_t c) { return c >= '0' && c <= '9'; }

// One token [p, e): TOK_INT ([+-]?[0-9]{1,18}: *iv, and *d as the converter gives it), TOK_DEC (*d), TOK_BAD (outside the token
// grammar) or TOK_RANGE (±inf, or a final decimal exponent above 308: pandas leaves the column as text).  *nint: the digits before
// the point.  More than 18 of them are outside the grammar in an integer token (pandas makes it int64 or uint64) and in a decimal
// token alike: pandas tries every column as int64 and then uint64 first, and where that attempt meets digits beyond uint64 before
// it meets a token with a point or an exponent -- "7" above "56963997270084518163.5" -- it leaves the column as text.
//
// The decimal value is pandas' default converter, not a correctly rounded one: the first 17 digits (leading zeros count) are
// accumulated in a double, later integer digits raise the exponent and later fraction digits are dropped; then one multiplication
// or division by an exact power of ten (two below 1e-308).  Every operation rounds on its own (-ffp-contract=off).
__host__ __device__ inline int parse_token(const uint8_t *p, const uint8_t *e, double *d, int64_t *iv, int *nint_out) {
#ifdef __HIP_DEVICE_COMPILE__
    const double *P = P10_DEV;
#else
    const double *P = P10_HOST;
#endif
    bool neg = false;
    if (p < e && (*p == '+' || *p == '-')) {
        neg = *p == '-';
        p++;
    }
    double num = 0.0;
    int exp = 0, nd = 0, ndec = 0, nint = 0, nfrac = 0;
    uint64_t acc = 0;
    for (; p < e && is_digit(*p); p++, nint++) {
        const int dg = *p - '0';
        if (nd < 17) {
            num = num * 10.0 + dg;
            nd++;
        } else {
            exp++;
        }
        if (nint < 18) acc = acc * 10 + dg;
    }
    bool dot = false, has_e = false;
    if (p < e && *p == '.') {
        dot = true;
        for (p++; p < e && is_digit(*p); p++, nfrac++) {
            if (nd < 17) {
                num = num * 10.0 + (*p - '0');
                nd++;
                ndec++;
            }
        }
    }
    if (nint + nfrac == 0) return TOK_BAD;
    int eval = 0;
    if (p < e && (*p == 'e' || *p == 'E')) {
        has_e = true;
        p++;
        int sgn = 1;
        if (p < e && (*p == '+' || *p == '-')) {
            sgn = *p == '-' ? -1 : 1;
            p++;
        }
        int k = 0;
        for (; p < e && is_digit(*p) && k < 4; p++, k++) eval = eval * 10 + (*p - '0');
        if (k == 0) return TOK_BAD;
        eval *= sgn;
    }
    if (p != e) return TOK_BAD;
    const bool integer = !dot && !has_e;
    if (nint > 18) return TOK_BAD;
    *nint_out = nint;
    if (integer) *iv = neg ? -(int64_t)acc : (int64_t)acc;
    exp -= ndec;
    if (neg) num = -num;
    exp += eval;
    if (exp > 308) return TOK_RANGE;
    if (exp > 0) num *= P[exp];
    else if (exp < -308) num = exp < -616 ? 0.0 : (num / P[-308 - exp]) / P[308];
    else num /= P[-exp];
    if (isinf(num)) return TOK_RANGE;
    *d = num;
    return integer ? TOK_INT : TOK_DEC;
}

// (text_scan.h: note_error, wg_scan, the 64 KiB blocks of the line pass -- a thread owns 16 consecutive 16-byte slices --, byte_of)

// WRITE = false: blk_cnt[b] := '\n' count of block b within [d0, N), and the first byte outside the grammar.
// WRITE = true: ends[blk_off[b] + rank] := the position of every '\n' of block b.
template <bool WRITE>
__global__ __launch_bounds__(WG) void tbl_lines(const uint8_t *T, int64_t d0, int64_t N, uint8_t sep, int *blk_cnt,
                                                const int64_t *blk_off, int64_t *ends, unsigned long long *err) {
    const int64_t base = blockIdx.x * NL_BLOCK + (int64_t)threadIdx.x * (NL_SLICES * 16);
    int cnt = 0;
    int64_t bad = -1;
    int bad_kind = 0;
    for (int j = 0; j < NL_SLICES; j++) {
        const int64_t p0 = base + j * 16;
        if (p0 >= N) break;
        const uint4 v = *reinterpret_cast<const uint4 *>(T + p0);
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const int64_t pos = p0 + k;
            const uint8_t c = byte_of(v, k);
            if (pos < d0 || pos >= N) continue;
            if (c == '\n') {
                cnt++;
            } else if (!WRITE && bad < 0) {
                if (c == '"') bad_kind = CYTO_TABLE_ERR_QUOTE;
                else if (c == '\r') bad_kind = (pos + 1 < N && T[pos + 1] == '\n') ? 0 : CYTO_TABLE_ERR_CR;
                else if (c < 0x20 && c != sep) bad_kind = CYTO_TABLE_ERR_BYTE;
                if (bad_kind) bad = pos;
            }
        }
    }
    if (!WRITE) {
        if (bad >= 0) note_error(err, bad, bad_kind);
        int tot;
        wg_scan(cnt, &tot);
        if (threadIdx.x == 0) blk_cnt[blockIdx.x] = tot;
        return;
    }
    int tot;
    int64_t out = blk_off[blockIdx.x] + wg_scan(cnt, &tot);
    for (int j = 0; j < NL_SLICES && cnt > 0; j++) {
        const int64_t p0 = base + j * 16;
        const uint4 v = *reinterpret_cast<const uint4 *>(T + p0);
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const int64_t pos = p0 + k;
            if (pos >= d0 && pos < N && byte_of(v, k) == '\n') {
                ends[out++] = pos;
                cnt--;
            }
        }
    }
}

// Data line g: [*s, *e) without its '\n' and a '\r' before it.
__device__ __forceinline__ void line_bounds(const uint8_t *T, const int64_t *ends, int64_t d0, int64_t g, int64_t *s, int64_t *e) {
    *s = g == 0 ? d0 : ends[g - 1] + 1;
    *e = ends[g];
    if (*e > *s && T[*e - 1] == '\r') (*e)--;
}

// A workgroup per data line.  Pass 1 (WRITE = false): every line has C delimiters, every token is in the grammar; dec[c] := 1 if
// column c has a decimal token, cast[c] := 1 if it has an integer token whose int64 value cast to float64 may differ from the
// converter's value (17 or 18 digits, or a negative zero: "-0" is 0 as an int64, -0.0 as a decimal); lab_len[g] := the label's length.
// Pass 2 (WRITE = true): out[g * C + c] := the int64 value, or the float64 bits where dec[c].
template <bool WRITE>
__global__ __launch_bounds__(WG) void tbl_fields(const uint8_t *T, const int64_t *ends, int64_t d0, int64_t C, uint8_t sep, int *dec,
                                                 int *cast, int64_t *lab_len, unsigned long long *err, int64_t *out) {
    const int64_t g = blockIdx.x;
    int64_t s, e;
    line_bounds(T, ends, d0, g, &s, &e);
    if (e == s) {
        if (!WRITE && threadIdx.x == 0) note_error(err, s, CYTO_TABLE_ERR_BLANK);
        return;
    }
    const int64_t a0 = s & ~(int64_t)15;
    const int64_t nsl = (e - a0 + 15) >> 4;
    int64_t done = 0;                                   // delimiters of the line in earlier rounds
    for (int64_t r0 = 0; r0 < nsl; r0 += WG) {
        const int64_t sl = r0 + threadIdx.x;
        const int64_t p0 = a0 + sl * 16;
        uint32_t mask = 0;
        if (sl < nsl) {
            const uint4 v = *reinterpret_cast<const uint4 *>(T + p0);
#pragma unroll
            for (int k = 0; k < 16; k++)
                if (p0 + k >= s && p0 + k < e && byte_of(v, k) == sep) mask |= 1u << k;
        }
        int tot;
        int64_t f = done + wg_scan(__popc(mask), &tot);   // delimiters before this slice: the column of the token after its first one
        while (mask) {
            const int k = __ffs(mask) - 1;
            mask &= mask - 1;
            const int64_t q = p0 + k;
            if (!WRITE && f == 0) lab_len[g] = q - s;
            if (f < C) {
                int64_t te = q + 1;
                while (te < e && T[te] != sep) te++;
                double d = 0.0;
                int64_t iv = 0;
                int nint = 0;
                const int kind = parse_token(T + q + 1, T + te, &d, &iv, &nint);
                if (!WRITE) {
                    if (kind == TOK_BAD) note_error(err, q + 1, CYTO_TABLE_ERR_TOKEN);
                    else if (kind == TOK_RANGE) note_error(err, q + 1, CYTO_TABLE_ERR_RANGE);
                    else if (kind == TOK_DEC) dec[f] = 1;
                    else if (nint >= 17 || (iv == 0 && signbit(d))) cast[f] = 1;
                } else {
                    out[g * C + f] = dec[f] ? (int64_t)__double_as_longlong(d) : iv;
                }
            }
            f++;
        }
        done += tot;
    }
    if (!WRITE && threadIdx.x == 0 && done != C) note_error(err, s, CYTO_TABLE_ERR_FIELDS);
}

// A thread per line: dst[lab_off[g] ...] := label, sep, '\n'.
__global__ __launch_bounds__(WG) void tbl_labels(const uint8_t *T, const int64_t *ends, int64_t d0, int64_t G, const int64_t *lab_len,
                                                 const int64_t *lab_off, uint8_t sep, uint8_t *dst) {
    const int64_t g = blockIdx.x * (int64_t)WG + threadIdx.x;
    if (g >= G) return;
    const int64_t s = g == 0 ? d0 : ends[g - 1] + 1, n = lab_len[g];
    uint8_t *o = dst + lab_off[g];
    for (int64_t i = 0; i < n; i++) o[i] = T[s + i];
    o[n] = sep;
    o[n + 1] = '\n';
}

// (Mem, cyto_common.h: the text and the result are as large as the input and do not go through the block cache; Pinned: the two
// chunk buffers of the streamed upload; text_scan.h: CHUNK, Fd, ms_since)

// The line of the file (1-based, the header being line 1) that holds byte `pos`; ends: the data lines' ends.
int64_t file_line(const std::vector<int64_t> &ends, int64_t pos) {
    int64_t lo = 0, hi = (int64_t)ends.size();
    while (lo < hi) {
        const int64_t m = (lo + hi) / 2;
        if (ends[m] < pos) lo = m + 1; else hi = m;
    }
    return lo + 2;
}

}  // namespace

struct cyto_table {
    int device_id = 0;
    int64_t G = 0, C = 0, label_bytes = 0;
    Mem values, dec, labels;
};

int cyto_table_read(const char *path, char sep, int64_t data_offset, int64_t ncols, int device_id, cyto_table **out, int64_t *shape,
                    int64_t *reason, double *ms) {
    if (!path || !out || !shape || !reason || ncols <= 0 || data_offset < 0 || (sep != ',' && sep != '\t')) return CYTO_ERR_BAD_ARG;
    *out = nullptr;
    reason[0] = reason[1] = reason[2] = 0;
    double t_read = 0, t_upload = 0, t_kernels = 0;
    auto refuse = [&](int kind, int64_t line, int64_t pos) {
        reason[0] = kind;
        reason[1] = line;
        reason[2] = pos;
        if (ms) ms[0] = t_read, ms[1] = t_upload, ms[2] = t_kernels;
        return (int)CYTO_ERR_UNSUPPORTED;
    };
    Fd f;
    struct stat sb;
    f.fd = open(path, O_RDONLY);
    if (f.fd < 0 || fstat(f.fd, &sb) != 0 || !S_ISREG(sb.st_mode)) return refuse(CYTO_TABLE_ERR_IO, 0, 0);
    const int64_t N = (int64_t)sb.st_size;
    if (data_offset >= N) return refuse(CYTO_TABLE_ERR_BLANK, 2, N);
    int rc;
    if ((rc = select_device(device_id))) return rc;
    const int64_t nblk = (N + NL_BLOCK - 1) / NL_BLOCK;
    const int64_t C = ncols;
    std::unique_ptr<cyto_table> t(new (std::nothrow) cyto_table);
    if (!t) return CYTO_ERR_NOMEM;
    t->device_id = device_id;
    t->C = C;
    // (declared before the stream: it drains before any buffer or copy source / destination is freed, whatever path leaves the call)
    Mem text, cnt, off, scal, ends, cast, len, loff;
    Pinned pin;
    Events<2> up;
    const unsigned long long no_err = ~0ull;
    unsigned long long e1 = no_err;
    int64_t hs[2] = {0, 0};
    std::vector<int64_t> hends, hlen, hoff;
    std::vector<int> hdec, hcast;
    StreamGuard sg;
    if ((rc = sg.acquire())) return rc;
    // scal: [0] the count of '\n', [1] the first error (byte << 8 | kind)
    if ((rc = text.alloc((size_t)(nblk * NL_BLOCK))) || (rc = cnt.alloc((size_t)nblk * 4)) || (rc = off.alloc((size_t)nblk * 8)) ||
        (rc = scal.alloc(16)))
        return rc;

    // (1) the file, streamed through two pinned buffers
    const auto t0 = std::chrono::steady_clock::now();
    if ((rc = up.create())) return rc;
    CYTO_HIP(hipHostMalloc(&pin.p[0], CHUNK, hipHostMallocDefault));
    CYTO_HIP(hipHostMalloc(&pin.p[1], CHUNK, hipHostMallocDefault));
    uint8_t last = 0;
    for (int64_t o = 0, k = 0; o < N; o += (int64_t)CHUNK, k++) {
        const int b = (int)(k & 1);
        if (k >= 2) CYTO_HIP(hipEventSynchronize(up[b]));
        const size_t n = (size_t)std::min<int64_t>((int64_t)CHUNK, N - o);
        const auto tr = std::chrono::steady_clock::now();
        size_t got = 0;
        while (got < n) {
            const ssize_t r = pread(f.fd, (char *)pin.p[b] + got, n - got, o + (int64_t)got);
            if (r <= 0) return refuse(CYTO_TABLE_ERR_IO, 0, o + (int64_t)got);
            got += (size_t)r;
        }
        t_read += ms_since(tr);
        last = ((const uint8_t *)pin.p[b])[n - 1];
        CYTO_HIP(hipMemcpyAsync(text.as<uint8_t>() + o, pin.p[b], n, hipMemcpyHostToDevice, sg.s));
        CYTO_HIP(hipEventRecord(up[b], sg.s));
    }
    CYTO_HIP(hipStreamSynchronize(sg.s));
    t_upload = ms_since(t0) - t_read;

    // (2) line ends
    const auto t1 = std::chrono::steady_clock::now();
    const uint8_t sp = (uint8_t)sep;
    CYTO_HIP(hipMemcpyAsync(scal.as<uint64_t>() + 1, &no_err, 8, hipMemcpyHostToDevice, sg.s));
    hipLaunchKernelGGL(tbl_lines<false>, dim3((unsigned)nblk), dim3(WG), 0, sg.s, text.as<uint8_t>(), data_offset, N, sp, cnt.as<int>(),
                       nullptr, nullptr, scal.as<unsigned long long>() + 1);
    CYTO_HIP(hipGetLastError());
    hipLaunchKernelGGL(tbl_scan_blocks, dim3(1), dim3(WG), 0, sg.s, cnt.as<int>(), nblk, off.as<int64_t>(), scal.as<int64_t>());
    CYTO_HIP(hipGetLastError());
    CYTO_HIP(hipMemcpyAsync(hs, scal.p, 16, hipMemcpyDeviceToHost, sg.s));
    CYTO_HIP(hipStreamSynchronize(sg.s));
    const int64_t G = hs[0] + (last != '\n' ? 1 : 0);   // a last line without its '\n' ends at N
    t->G = G;
    if ((rc = ends.alloc((size_t)G * 8))) return rc;
    hipLaunchKernelGGL(tbl_lines<true>, dim3((unsigned)nblk), dim3(WG), 0, sg.s, text.as<uint8_t>(), data_offset, N, sp, nullptr,
                       off.as<int64_t>(), ends.as<int64_t>(), nullptr);
    CYTO_HIP(hipGetLastError());
    if (last != '\n') CYTO_HIP(hipMemcpyAsync(ends.as<int64_t>() + hs[0], &N, 8, hipMemcpyHostToDevice, sg.s));
    auto fail_at = [&](unsigned long long e) -> int {
        hends.resize((size_t)G);
        CYTO_HIP(hipMemcpyAsync(hends.data(), ends.p, (size_t)G * 8, hipMemcpyDeviceToHost, sg.s));
        CYTO_HIP(hipStreamSynchronize(sg.s));
        t_kernels = ms_since(t1);
        const int64_t pos = (int64_t)(e >> 8);
        return refuse((int)(e & 0xff), file_line(hends, pos), pos);
    };
    if ((unsigned long long)hs[1] != no_err) return fail_at((unsigned long long)hs[1]);

    // (3) pass 1: field counts, tokens, column types, label lengths
    if ((rc = t->dec.alloc((size_t)C * 4)) || (rc = cast.alloc((size_t)C * 4)) || (rc = len.alloc((size_t)G * 8))) return rc;
    CYTO_HIP(hipMemsetAsync(t->dec.p, 0, (size_t)C * 4, sg.s));
    CYTO_HIP(hipMemsetAsync(cast.p, 0, (size_t)C * 4, sg.s));
    hipLaunchKernelGGL(tbl_fields<false>, dim3((unsigned)G), dim3(WG), 0, sg.s, text.as<uint8_t>(), ends.as<int64_t>(), data_offset, C,
                       sp, t->dec.as<int>(), cast.as<int>(), len.as<int64_t>(), scal.as<unsigned long long>() + 1, nullptr);
    CYTO_HIP(hipGetLastError());
    hdec.resize((size_t)C);
    hcast.resize((size_t)C);
    hlen.resize((size_t)G);
    hoff.resize((size_t)G);
    CYTO_HIP(hipMemcpyAsync(&e1, scal.as<uint64_t>() + 1, 8, hipMemcpyDeviceToHost, sg.s));
    CYTO_HIP(hipMemcpyAsync(hdec.data(), t->dec.p, (size_t)C * 4, hipMemcpyDeviceToHost, sg.s));
    CYTO_HIP(hipMemcpyAsync(hcast.data(), cast.p, (size_t)C * 4, hipMemcpyDeviceToHost, sg.s));
    CYTO_HIP(hipMemcpyAsync(hlen.data(), len.p, (size_t)G * 8, hipMemcpyDeviceToHost, sg.s));
    CYTO_HIP(hipStreamSynchronize(sg.s));
    if (e1 != no_err) return fail_at(e1);
    // pandas converts a column a block of rows at a time (low_memory): a block without a decimal token becomes int64, cast to float64
    // when the blocks are joined.  An integer token of a float64 column whose cast may differ from the converter's value is refused.
    for (int64_t c = 0; c < C; c++)
        if (hdec[(size_t)c] && hcast[(size_t)c]) {
            t_kernels = ms_since(t1);
            return refuse(CYTO_TABLE_ERR_INT_CAST, 0, c);
        }

    // (4) pass 2: the values; the labels
    int64_t lb = 0;
    for (int64_t g = 0; g < G; g++) {
        hoff[(size_t)g] = lb;
        lb += hlen[(size_t)g] + 2;
    }
    t->label_bytes = lb;
    if ((rc = t->values.alloc((size_t)(G * C) * 8)) || (rc = t->labels.alloc((size_t)lb)) || (rc = loff.alloc((size_t)G * 8))) return rc;
    hipLaunchKernelGGL(tbl_fields<true>, dim3((unsigned)G), dim3(WG), 0, sg.s, text.as<uint8_t>(), ends.as<int64_t>(), data_offset, C,
                       sp, t->dec.as<int>(), nullptr, nullptr, nullptr, t->values.as<int64_t>());
    CYTO_HIP(hipGetLastError());
    CYTO_HIP(hipMemcpyAsync(loff.p, hoff.data(), (size_t)G * 8, hipMemcpyHostToDevice, sg.s));
    hipLaunchKernelGGL(tbl_labels, dim3((unsigned)((G + WG - 1) / WG)), dim3(WG), 0, sg.s, text.as<uint8_t>(), ends.as<int64_t>(),
                       data_offset, G, len.as<int64_t>(), loff.as<int64_t>(), sp, t->labels.as<uint8_t>());
    CYTO_HIP(hipGetLastError());
    CYTO_HIP(hipStreamSynchronize(sg.s));
    t_kernels = ms_since(t1);
    shape[0] = G;
    shape[1] = C;
    shape[2] = lb;
    if (ms) ms[0] = t_read, ms[1] = t_upload, ms[2] = t_kernels;
    *out = t.release();
    return CYTO_OK;
}

int cyto_table_fetch(cyto_table *t, int64_t *values, int8_t *col_is_float, char *labels, double *ms_download) {
    if (!t || !values || !col_is_float || !labels) return CYTO_ERR_BAD_ARG;
    int rc;
    if ((rc = select_device(t->device_id))) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<int> dec((size_t)t->C);
    CYTO_HIP(hipMemcpy(values, t->values.p, (size_t)(t->G * t->C) * 8, hipMemcpyDeviceToHost));
    CYTO_HIP(hipMemcpy(dec.data(), t->dec.p, (size_t)t->C * 4, hipMemcpyDeviceToHost));
    CYTO_HIP(hipMemcpy(labels, t->labels.p, (size_t)t->label_bytes, hipMemcpyDeviceToHost));
    for (int64_t c = 0; c < t->C; c++) col_is_float[c] = (int8_t)(dec[(size_t)c] != 0);
    if (ms_download) *ms_download = ms_since(t0);
    return CYTO_OK;
}

int cyto_table_values(cyto_table *t, const void **values_dev, int64_t *ld) {
    if (!t || !values_dev || !ld) return CYTO_ERR_BAD_ARG;
    *values_dev = t->values.p;
    *ld = t->C;
    return CYTO_OK;
}

int cyto_table_fetch_labels(cyto_table *t, int8_t *col_is_float, char *labels, double *ms_download) {
    if (!t || !col_is_float || !labels) return CYTO_ERR_BAD_ARG;
    int rc;
    if ((rc = select_device(t->device_id))) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<int> dec((size_t)t->C);
    CYTO_HIP(hipMemcpy(dec.data(), t->dec.p, (size_t)t->C * 4, hipMemcpyDeviceToHost));
    CYTO_HIP(hipMemcpy(labels, t->labels.p, (size_t)t->label_bytes, hipMemcpyDeviceToHost));
    for (int64_t c = 0; c < t->C; c++) col_is_float[c] = (int8_t)(dec[(size_t)c] != 0);
    if (ms_download) *ms_download = ms_since(t0);
    return CYTO_OK;
}

void cyto_table_free(cyto_table *t) {
    if (t && select_device(t->device_id) == CYTO_OK) delete t;
}

int cyto_table_parse_tokens(const char *text, int64_t n, const int64_t *offsets, double *values, int64_t *ints, int8_t *kinds) {
    if (n < 0 || (n > 0 && (!text || !offsets || !values || !ints || !kinds))) return CYTO_ERR_BAD_ARG;
    const uint8_t *u = reinterpret_cast<const uint8_t *>(text);
    for (int64_t i = 0; i < n; i++) {
        double d = 0.0;
        int64_t iv = 0;
        int nint = 0;
        kinds[i] = (int8_t)parse_token(u + offsets[i], u + offsets[i + 1], &d, &iv, &nint);
        values[i] = d;
        ints[i] = iv;
    }
    return CYTO_OK;
}
