// mtx_read.hip -- the body of a MatrixMarket coordinate file (common.py:read_mtx_device) parsed and scattered into a dense G x C
// matrix on the device, value for value what scipy.io.mmread(path).toarray() holds, or refused (CYTO_ERR_UNSUPPORTED) so that the
// caller reads the file with scipy.  DESIGN.md 4.1e has the grammar and the reason for every refusal.
//
// The caller parses the banner, the comments and the size line and passes where the entry lines start, the shape and nnz.
//   upload        as in table.hip: 16 MiB chunks through two pinned buffers, each uploaded while the next one is read.
//   mtxr_lines    (a workgroup per 64 KiB) counts the '\n' of the body and checks its bytes: only digits - . e E + space tab, '\n',
//                 and '\r' before '\n'; no blank as the file's last byte.  tbl_scan_blocks turns the block counts into offsets and
//                 mtxr_lines<true> writes the line ends.
//   mtxr_entries  (a thread per line) splits the line into its three tokens, checks the indices and converts the value with
//                 parse_entry -- the function the host hook cyto_mtx_parse_entries runs -- and scatters into the zero-filled result:
//                 integer values with a 64-bit atomicAdd (duplicates sum, exactly and in any order), real values with an atomicExch
//                 whose non-zero old value gives a duplicate away.
//   mtxr_dups     runs only after a real file showed a duplicate: it names the refusal's line independently of the launch order.
#include "text_scan.h"

#include <fcntl.h>
#include <sys/stat.h>

#include <algorithm>
#include <vector>

namespace {

using namespace cyto;

#define CYTO_P10_22 1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22

// The powers of ten that a double holds exactly.  (each side of the compilation uses one of the two)
[[maybe_unused]] __constant__ double P10_DEV[23] = {CYTO_P10_22};
[[maybe_unused]] const double P10_HOST[23] = {CYTO_P10_22};

__host__ __device__ inline bool is_digit(uint8_t c) { return c >= '0' && c <= '9'; }
__host__ __device__ inline bool is_blank(uint8_t c) { return c == ' ' || c == '\t'; }

// An index token [p, e): [0-9]{1,18} with 1 <= value <= lim.
__host__ __device__ inline bool parse_index(const uint8_t *p, const uint8_t *e, int64_t lim, int64_t *out) {
    if (e - p < 1 || e - p > 18) return false;
    int64_t v = 0;
    for (; p < e; p++) {
        if (!is_digit(*p)) return false;
        v = v * 10 + (*p - '0');
    }
    *out = v;
    return v >= 1 && v <= lim;
}

// An integer-field value [p, e): -?[0-9]{1,18}.  0 or CYTO_MTXR_ERR_TOKEN.
__host__ __device__ inline int parse_int_value(const uint8_t *p, const uint8_t *e, int64_t *out) {
    const bool neg = p < e && *p == '-';
    if (neg) p++;
    if (e - p < 1 || e - p > 18) return CYTO_MTXR_ERR_TOKEN;
    int64_t v = 0;
    for (; p < e; p++) {
        if (!is_digit(*p)) return CYTO_MTXR_ERR_TOKEN;
        v = v * 10 + (*p - '0');
    }
    *out = neg ? -v : v;
    return 0;
}

// A real-field value [p, e): -? digits with at most one point and at least one digit, then optionally [eE][+-]?[0-9]{1,4}.  The
// fraction's trailing zeros are dropped; w: the remaining digits as an integer, ex: the exponent minus the fraction digits kept.
// Inside the window w < 10^15, |ex| <= 22 both w and 10^|ex| are exact doubles, so the one multiplication or division is the
// correctly rounded value of the token -- what scipy's converter returns.  *out: the float64 bits.
// 0, CYTO_MTXR_ERR_TOKEN, _INEXACT (outside the window) or _NEGZERO (a zero with a minus sign: scipy's dense result holds +0.0).
__host__ __device__ inline int parse_real_value(const uint8_t *p, const uint8_t *e, int64_t *out) {
#ifdef __HIP_DEVICE_COMPILE__
    const double *P = P10_DEV;
#else
    const double *P = P10_HOST;
#endif
    const uint64_t W_MAX = 1000000000000000ull;         // 10^15
    const bool neg = p < e && *p == '-';
    if (neg) p++;
    uint64_t w = 0;
    bool wide = false;
    bool any = false;
    // pending: fraction zeros not (yet) followed by another digit.  Both counts stop at SAT: a token with that many fraction digits
    // is outside the window whatever the rest of it says (the exponent has at most four digits).
    const int SAT = 1000000;
    int nfrac = 0, pending = 0;
    for (; p < e && is_digit(*p); p++, any = true) {
        if (!wide) w = w * 10 + (uint64_t)(*p - '0');
        wide = wide || w >= W_MAX;
    }
    if (p < e && *p == '.') {
        for (p++; p < e && is_digit(*p); p++, any = true) {
            if (*p == '0') {
                pending += pending < SAT;
                continue;
            }
            for (int z = pending; z >= 0; z--) {        // the zeros held back, then this digit
                if (!wide) w = w * 10 + (uint64_t)(z ? 0 : *p - '0');
                wide = wide || w >= W_MAX;
                nfrac += nfrac < SAT;
            }
            pending = 0;
        }
    }
    if (!any) return CYTO_MTXR_ERR_TOKEN;
    int ex = 0;
    if (p < e && (*p == 'e' || *p == 'E')) {
        p++;
        bool eneg = false;
        if (p < e && (*p == '+' || *p == '-')) {
            eneg = *p == '-';
            p++;
        }
        int k = 0;
        for (; p < e && is_digit(*p) && k < 4; p++, k++) ex = ex * 10 + (*p - '0');
        if (k == 0) return CYTO_MTXR_ERR_TOKEN;
        if (eneg) ex = -ex;
    }
    if (p != e) return CYTO_MTXR_ERR_TOKEN;
    ex -= nfrac;
    if (wide || ex > 22 || ex < -22) return CYTO_MTXR_ERR_INEXACT;
    if (w == 0) {
        if (neg) return CYTO_MTXR_ERR_NEGZERO;
        *out = 0;
        return 0;
    }
    double d = (double)w;
    d = ex >= 0 ? d * P[ex] : d / P[-ex];
    if (neg) d = -d;
    memcpy(out, &d, 8);
    return 0;
}

// An entry line [p, e), without its line end: optional blanks, three tokens separated by blanks, optional blanks.  0 with *row,
// *col (1-based) and *val (the int64 value or the float64 bits), or a CYTO_MTXR_ERR_* with *where := the offset in the line that
// the refusal names: 0 for an empty line and a wrong token count, else the first byte of the first token outside its grammar.
__host__ __device__ inline int parse_entry(const uint8_t *p, const uint8_t *e, int field, int64_t G, int64_t C, int64_t *row,
                                           int64_t *col, int64_t *val, int64_t *where) {
    *where = 0;
    if (p == e) return CYTO_MTXR_ERR_BLANK;
    const uint8_t *q = p, *t0[3], *t1[3];
    for (int k = 0; k < 3; k++) {
        while (q < e && is_blank(*q)) q++;
        if (q == e) return CYTO_MTXR_ERR_FIELDS;
        t0[k] = q;
        while (q < e && !is_blank(*q)) q++;
        t1[k] = q;
    }
    while (q < e && is_blank(*q)) q++;
    if (q != e) return CYTO_MTXR_ERR_FIELDS;
    *where = t0[0] - p;
    if (!parse_index(t0[0], t1[0], G, row)) return CYTO_MTXR_ERR_INDEX;
    *where = t0[1] - p;
    if (!parse_index(t0[1], t1[1], C, col)) return CYTO_MTXR_ERR_INDEX;
    *where = t0[2] - p;
    return field == 0 ? parse_int_value(t0[2], t1[2], val) : parse_real_value(t0[2], t1[2], val);
}

// WRITE = false: blk_cnt[b] := '\n' count of block b within [d0, N), and the first byte outside the grammar.
// WRITE = true: ends[blk_off[b] + rank] := the position of every '\n' of block b.
template <bool WRITE>
__global__ __launch_bounds__(WG) void mtxr_lines(const uint8_t *T, int64_t d0, int64_t N, int *blk_cnt, const int64_t *blk_off,
                                                 int64_t *ends, unsigned long long *err) {
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
                if (c == '\r') bad_kind = (pos + 1 < N && T[pos + 1] == '\n') ? 0 : CYTO_MTXR_ERR_CR;
                else if (!(is_digit(c) || is_blank(c) || c == '-' || c == '.' || c == 'e' || c == 'E' || c == '+') ||
                         (is_blank(c) && pos == N - 1))      // (a blank that ends the file: scipy 1.15 reads beyond it)
                    bad_kind = CYTO_MTXR_ERR_BYTE;
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

// Entry line i: [*s, *e) without its '\n' and a '\r' before it.
__device__ __forceinline__ void entry_bounds(const uint8_t *T, const int64_t *ends, int64_t d0, int64_t i, int64_t *s, int64_t *e) {
    *s = i == 0 ? d0 : ends[i - 1] + 1;
    *e = ends[i];
    if (*e > *s && T[*e - 1] == '\r') (*e)--;
}

// A thread per entry line.  res: G x C words, zero on entry.  FIELD 0: res[row, col] += value (int64, wrapping); FIELD 1:
// res[row, col] := the float64 bits of a non-zero value.  *dups += 1 for every entry that found its cell non-zero.  A zero value
// leaves its cell alone (0 + x = x), so neither the sums nor what counts as a duplicate depend on the order of the threads.
template <int FIELD>
__global__ __launch_bounds__(WG) void mtxr_entries(const uint8_t *T, const int64_t *ends, int64_t d0, int64_t nnz, int64_t G, int64_t C,
                                                   unsigned long long *res, unsigned long long *err, unsigned long long *dups) {
    const int64_t i = blockIdx.x * (int64_t)WG + threadIdx.x;
    if (i >= nnz) return;
    int64_t s, e, row = 0, col = 0, val = 0, where = 0;
    entry_bounds(T, ends, d0, i, &s, &e);
    const int kind = parse_entry(T + s, T + e, FIELD, G, C, &row, &col, &val, &where);
    if (kind) {
        note_error(err, s + where, kind);
        return;
    }
    if (val == 0) return;
    unsigned long long *cell = res + ((row - 1) * C + (col - 1));
    const unsigned long long old = FIELD == 0 ? atomicAdd(cell, (unsigned long long)val) : atomicExch(cell, (unsigned long long)val);
    if (old != 0) atomicAdd(dups, 1ull);
}

// After a real file showed a duplicate.  res: G x C words, all ones on entry; every non-zero entry takes the minimum of its line
// number into its cell.  Of the lines l1 < l2 < ... of one cell, whichever order they arrive in, some thread sees the pair
// (l1, l2) and none sees a pair whose later line is below l2: the refusal is the first byte of the lowest such l2.
__global__ __launch_bounds__(WG) void mtxr_dups(const uint8_t *T, const int64_t *ends, int64_t d0, int64_t nnz, int64_t G, int64_t C,
                                                unsigned long long *res, unsigned long long *err) {
    const int64_t i = blockIdx.x * (int64_t)WG + threadIdx.x;
    if (i >= nnz) return;
    int64_t s, e, row = 0, col = 0, val = 0, where = 0;
    entry_bounds(T, ends, d0, i, &s, &e);
    if (parse_entry(T + s, T + e, 1, G, C, &row, &col, &val, &where) || val == 0) return;
    const unsigned long long old = atomicMin(res + ((row - 1) * C + (col - 1)), (unsigned long long)i);
    if (old == ~0ull) return;
    const int64_t later = i > (int64_t)old ? i : (int64_t)old;
    note_error(err, ends[later - 1] + 1, CYTO_MTXR_ERR_DUPLICATE);      // (later >= 1: two distinct lines)
}

}  // namespace

int cyto_mtx_read(const char *path, int64_t data_offset, int64_t G, int64_t C, int64_t nnz, int field, int64_t *out, int64_t ldo,
                  int device_id, cyto_mtx_read_info *info) {
    if (!path || !out || !info || G <= 0 || C <= 0 || nnz < 0 || data_offset < 0 || ldo < C || (field != 0 && field != 1))
        return CYTO_ERR_BAD_ARG;
    memset(info, 0, sizeof *info);
    double t_read = 0, t_upload = 0, t_kernels = 0;
    auto refuse = [&](int kind, int64_t line, int64_t pos) {
        info->reason_kind = kind;
        info->reason_line = line;
        info->reason_byte = pos;
        info->ms_read = t_read, info->ms_upload = t_upload, info->ms_kernels = t_kernels;
        return (int)CYTO_ERR_UNSUPPORTED;
    };
    Fd f;
    struct stat sb;
    f.fd = open(path, O_RDONLY);
    if (f.fd < 0 || fstat(f.fd, &sb) != 0 || !S_ISREG(sb.st_mode) || (int64_t)sb.st_size < data_offset)
        return refuse(CYTO_MTXR_ERR_IO, 0, 0);
    const int64_t N = (int64_t)sb.st_size;
    if (G > (INT64_MAX / 8) / C) return refuse(CYTO_MTXR_ERR_MEMORY, 0, 0);
    int rc;
    if ((rc = select_device(device_id))) return rc;
    const int64_t nblk = std::max<int64_t>(1, (N + NL_BLOCK - 1) / NL_BLOCK);
    const size_t res_bytes = (size_t)(G * C) * 8;
    size_t mem_free = 0, mem_total = 0;
    CYTO_HIP(hipMemGetInfo(&mem_free, &mem_total));
    // (the text, the result, the line ends -- at most one per two bytes of a body without empty lines, and nnz of them --, some room)
    if ((double)(nblk * NL_BLOCK) + (double)res_bytes + 8.0 * (double)std::min(N / 2 + 1, nnz + 1) + double(64 << 20) > (double)mem_free)
        return refuse(CYTO_MTXR_ERR_MEMORY, 0, 0);
    // (declared before the stream: it drains before any buffer or copy source / destination is freed, whatever path leaves the call)
    Mem text, res;
    DevBuf cnt, off, scal, ends;
    Pinned pin;
    Events<2> up;
    const unsigned long long no_err = ~0ull;
    unsigned long long hs[3] = {0, 0, 0};
    std::vector<int64_t> hends;
    StreamGuard sg;
    if ((rc = sg.acquire())) return rc;
    auto no_room = [&](int st) { return st == CYTO_ERR_NOMEM ? refuse(CYTO_MTXR_ERR_MEMORY, 0, 0) : st; };
    // scal: [0] the count of '\n', [1] the first error (byte << 8 | kind), [2] duplicates
    if ((rc = text.alloc((size_t)(nblk * NL_BLOCK))) || (rc = res.alloc(res_bytes)) || (rc = cnt.alloc((size_t)nblk * 4, sg.s)) ||
        (rc = off.alloc((size_t)nblk * 8, sg.s)) || (rc = scal.alloc(24, sg.s)))
        return no_room(rc);

    // (1) the file, streamed through two pinned buffers; the '\n' before the body give the file's line numbers
    const auto t0 = std::chrono::steady_clock::now();
    if ((rc = up.create())) return rc;
    CYTO_HIP(hipHostMalloc(&pin.p[0], CHUNK, hipHostMallocDefault));
    CYTO_HIP(hipHostMalloc(&pin.p[1], CHUNK, hipHostMallocDefault));
    uint8_t last = 0;
    int64_t head_lines = 0;
    for (int64_t o = 0, k = 0; o < N; o += (int64_t)CHUNK, k++) {
        const int b = (int)(k & 1);
        if (k >= 2) CYTO_HIP(hipEventSynchronize(up[b]));
        const size_t n = (size_t)std::min<int64_t>((int64_t)CHUNK, N - o);
        const auto tr = std::chrono::steady_clock::now();
        size_t got = 0;
        while (got < n) {
            const ssize_t r = pread(f.fd, (char *)pin.p[b] + got, n - got, o + (int64_t)got);
            if (r <= 0) return refuse(CYTO_MTXR_ERR_IO, 0, o + (int64_t)got);
            got += (size_t)r;
        }
        t_read += ms_since(tr);
        const uint8_t *h = (const uint8_t *)pin.p[b];
        last = h[n - 1];
        if (o < data_offset) head_lines += std::count(h, h + std::min<int64_t>((int64_t)n, data_offset - o), (uint8_t)'\n');
        CYTO_HIP(hipMemcpyAsync(text.as<uint8_t>() + o, pin.p[b], n, hipMemcpyHostToDevice, sg.s));
        CYTO_HIP(hipEventRecord(up[b], sg.s));
    }
    CYTO_HIP(hipStreamSynchronize(sg.s));
    t_upload = ms_since(t0) - t_read;

    // (2) the zero fill of the result; line ends and the byte check
    const auto t1 = std::chrono::steady_clock::now();
    unsigned long long *err = scal.as<unsigned long long>() + 1, *dups = scal.as<unsigned long long>() + 2;
    const unsigned long long init[3] = {0, no_err, 0};
    CYTO_HIP(hipMemsetAsync(res.p, 0, res_bytes, sg.s));
    CYTO_HIP(hipMemcpyAsync(scal.p, init, 24, hipMemcpyHostToDevice, sg.s));
    hipLaunchKernelGGL(mtxr_lines<false>, dim3((unsigned)nblk), dim3(WG), 0, sg.s, text.as<uint8_t>(), data_offset, N, cnt.as<int>(),
                       nullptr, nullptr, err);
    CYTO_HIP(hipGetLastError());
    hipLaunchKernelGGL(tbl_scan_blocks, dim3(1), dim3(WG), 0, sg.s, cnt.as<int>(), nblk, off.as<int64_t>(), scal.as<int64_t>());
    CYTO_HIP(hipGetLastError());
    CYTO_HIP(hipMemcpyAsync(hs, scal.p, 16, hipMemcpyDeviceToHost, sg.s));
    CYTO_HIP(hipStreamSynchronize(sg.s));
    const bool open_end = N > data_offset && last != '\n';      // a last line without its '\n' ends at N
    const int64_t L = (int64_t)hs[0] + (open_end ? 1 : 0);
    if (hs[1] == no_err && L != nnz) {
        t_kernels = ms_since(t1);
        return refuse(CYTO_MTXR_ERR_COUNT, 0, L);
    }
    if ((rc = ends.alloc((size_t)L * 8, sg.s))) return no_room(rc);
    hipLaunchKernelGGL(mtxr_lines<true>, dim3((unsigned)nblk), dim3(WG), 0, sg.s, text.as<uint8_t>(), data_offset, N, nullptr,
                       off.as<int64_t>(), ends.as<int64_t>(), nullptr);
    CYTO_HIP(hipGetLastError());
    if (open_end) CYTO_HIP(hipMemcpyAsync(ends.as<int64_t>() + hs[0], &N, 8, hipMemcpyHostToDevice, sg.s));
    auto fail_at = [&](unsigned long long e) -> int {
        hends.resize((size_t)L);
        if (L > 0) CYTO_HIP(hipMemcpyAsync(hends.data(), ends.p, (size_t)L * 8, hipMemcpyDeviceToHost, sg.s));
        CYTO_HIP(hipStreamSynchronize(sg.s));
        t_kernels = ms_since(t1);
        const int64_t pos = (int64_t)(e >> 8);
        const int64_t below = std::lower_bound(hends.begin(), hends.end(), pos) - hends.begin();     // line ends below pos
        return refuse((int)(e & 0xff), head_lines + below + 1, pos);
    };
    if (hs[1] != no_err) return fail_at(hs[1]);

    // (3) the entries
    if (nnz > 0) {
        const dim3 grid((unsigned)((nnz + WG - 1) / WG));
        if (field == 0)
            hipLaunchKernelGGL(mtxr_entries<0>, grid, dim3(WG), 0, sg.s, text.as<uint8_t>(), ends.as<int64_t>(), data_offset, nnz, G, C,
                               res.as<unsigned long long>(), err, dups);
        else
            hipLaunchKernelGGL(mtxr_entries<1>, grid, dim3(WG), 0, sg.s, text.as<uint8_t>(), ends.as<int64_t>(), data_offset, nnz, G, C,
                               res.as<unsigned long long>(), err, dups);
        CYTO_HIP(hipGetLastError());
        CYTO_HIP(hipMemcpyAsync(hs + 1, err, 16, hipMemcpyDeviceToHost, sg.s));
        CYTO_HIP(hipStreamSynchronize(sg.s));
        if (hs[1] != no_err) return fail_at(hs[1]);
        if (field == 1 && hs[2] != 0) {
            CYTO_HIP(hipMemsetAsync(res.p, 0xff, res_bytes, sg.s));
            hipLaunchKernelGGL(mtxr_dups, grid, dim3(WG), 0, sg.s, text.as<uint8_t>(), ends.as<int64_t>(), data_offset, nnz, G, C,
                               res.as<unsigned long long>(), err);
            CYTO_HIP(hipGetLastError());
            CYTO_HIP(hipMemcpyAsync(hs + 1, err, 8, hipMemcpyDeviceToHost, sg.s));
            CYTO_HIP(hipStreamSynchronize(sg.s));
            return hs[1] != no_err ? fail_at(hs[1]) : (int)CYTO_ERR_INTERNAL;
        }
    }
    t_kernels = ms_since(t1);

    // (4) the dense result
    const auto t2 = std::chrono::steady_clock::now();
    if (ldo == C) CYTO_HIP(hipMemcpyAsync(out, res.p, res_bytes, hipMemcpyDeviceToHost, sg.s));
    else CYTO_HIP(hipMemcpy2DAsync(out, (size_t)ldo * 8, res.p, (size_t)C * 8, (size_t)C * 8, (size_t)G, hipMemcpyDeviceToHost, sg.s));
    CYTO_HIP(hipStreamSynchronize(sg.s));
    info->ms_download = ms_since(t2);
    info->entries = nnz;
    info->duplicates = (int64_t)hs[2];
    info->ms_read = t_read, info->ms_upload = t_upload, info->ms_kernels = t_kernels;
    return CYTO_OK;
}

int cyto_mtx_parse_entries(const char *text, int64_t n, const int64_t *offsets, int field, int64_t G, int64_t C, int8_t *kinds,
                           int64_t *where, int64_t *rows, int64_t *cols, int64_t *values) {
    if (n < 0 || (field != 0 && field != 1) || (n > 0 && (!text || !offsets || !kinds || !where || !rows || !cols || !values)))
        return CYTO_ERR_BAD_ARG;
    const uint8_t *u = reinterpret_cast<const uint8_t *>(text);
    for (int64_t i = 0; i < n; i++) {
        rows[i] = cols[i] = values[i] = 0;
        kinds[i] = (int8_t)parse_entry(u + offsets[i], u + offsets[i + 1], field, G, C, &rows[i], &cols[i], &values[i], &where[i]);
    }
    return CYTO_OK;
}
