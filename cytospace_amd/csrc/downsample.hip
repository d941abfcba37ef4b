// downsample.hip -- common.py:downsample on the device, draw for draw the same as numpy's legacy global RandomState.
//
// The host function draws, cell by cell in column order, `np.random.choice(np.repeat(genes, col), target)`: with replacement
// that is randint(0, T) for the cell's total T, i.e. 32-bit MT19937 words w taken until (w & mask) <= T-1 (mask: the smallest
// 2^k - 1 >= T-1), and the draw r selects the gene g with cumsum[g-1] <= r < cumsum[g].  Cells with T <= target are kept and
// take no words.
//
//   stage 1 (ds_stream, ONE wave): the MT19937 stream and the acceptance test.  The twist runs in place on numpy's key[624]
//            in three slices [0,227) [227,454) [454,624): within a slice every new word depends on words of earlier slices
//            only (x[k+624] = x[k+397] ^ twist(x[k], x[k+1])), so a slice is computed lane-parallel.  Words are tested 64 at a
//            time with a ballot; the accepted r go to the cell's target-wide row of rbuf.  When a cell's target is reached
//            inside a group of 64, the rest of the group is tested again with the next cell's mask.
//   stage 2 (ds_hist, a workgroup per downsampled cell): the column's cumulative counts, a chunk of genes at a time in LDS;
//            every r of the cell that falls into the chunk is placed by an upper-bound search and counted in an LDS
//            histogram, which is written out as the cell's new column.
//
// Columns that are not downsampled are copied by ds_copy.  Cells are processed in blocks whose r rows fit in ~1 GiB; stage 1
// of block b+1 (its own stream) overlaps stage 2 of block b (double-buffered rbuf).
//
// cyto_placeholders (the "place_holders" sampler's synthetic cells) runs the same stage 1 -- a synthetic cell is a "cell" with
// range n - 1 and G accepted draws -- with ph_gather as its stage 2.
#include "cyto_common.h"

#include <algorithm>
#include <vector>

namespace {

using namespace cyto;

constexpr int MT_N = 624, MT_M = 397;
constexpr int SLICE_LO[3] = {0, 227, 454};
constexpr int SLICE_HI[3] = {227, 454, 624};

// Stage 1's persistent state between blocks: numpy's (key, pos) and the words consumed so far.
struct MtState {
    uint32_t key[MT_N];
    uint32_t pos;
    uint32_t pad;
    unsigned long long words;
};

__device__ __forceinline__ uint32_t temper(uint32_t y) {
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
}

__device__ __forceinline__ uint32_t gen_mask(uint32_t rng) { return rng ? (0xffffffffu >> __clz(rng)) : 0u; }

// Recompute key[lo, hi) in place (numpy's mt19937_gen order).  Every read of the slice happens before any write of it: a
// lane's key[i+1] is another lane's key[i].
__device__ __forceinline__ void twist_slice(uint32_t *key, int lo, int hi) {
    const int lane = threadIdx.x;
    uint32_t v[4];
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const int i = lo + t * 64 + lane;
        if (i < hi) {
            const int i1 = i + 1 == MT_N ? 0 : i + 1;
            const int im = i + MT_M >= MT_N ? i + MT_M - MT_N : i + MT_M;
            const uint32_t y = (key[i] & 0x80000000u) | (key[i1] & 0x7fffffffu);
            v[t] = key[im] ^ (y >> 1) ^ ((0u - (y & 1u)) & 0x9908b0dfu);
        }
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const int i = lo + t * 64 + lane;
        if (i < hi) key[i] = v[t];
    }
    __syncthreads();
}

// rngs[d] = T_d - 1 for the nd downsampled cells of this block (in column order); each gets `target` accepted draws in
// rbuf[d * target ...].  The stream continues from st (numpy's key/pos); on return st holds numpy's state after the last
// consumed word (pos == 624 with the twist deferred when that word ends the key).
__global__ __launch_bounds__(64) void ds_stream(MtState *st, const uint32_t *rngs, int nd, int target, uint32_t *rbuf) {
    __shared__ uint32_t key[MT_N];
    const int lane = threadIdx.x;
    for (int i = lane; i < MT_N; i += 64) key[i] = st->key[i];
    const int pos0 = (int)st->pos;
    __syncthreads();
    if (nd <= 0 || target <= 0) return;

    int d = 0, k = 0, end = pos0;
    uint32_t rng = rngs[0], mask = gen_mask(rng);
    unsigned long long used = 0;
    int slice = pos0 >= MT_N ? 0 : -1;            // -1: the rest of the current key, key[pos0:]
    bool done = false;
    const unsigned long long below = (1ull << lane) - 1ull;
    while (!done) {
        int lo = pos0, hi = MT_N;
        if (slice >= 0) {
            lo = SLICE_LO[slice];
            hi = SLICE_HI[slice];
            twist_slice(key, lo, hi);
        }
        int s = lo;
        while (s < hi) {
            const int i = s + lane;
            const bool valid = i < hi;
            const uint32_t r = valid ? (temper(key[i]) & mask) : 0u;
            const bool acc = valid && r <= rng;
            const unsigned long long b = __ballot(acc);
            const int n = __popcll(b);
            const int rank = __popcll(b & below);
            const int need = target - k;
            uint32_t *row = rbuf + (size_t)d * target + k;
            if (n < need) {
                if (acc) row[rank] = r;
                k += n;
                s += 64;
                continue;
            }
            // the need-th accept ends this cell; the words after it belong to the next one
            const unsigned long long cut = __ballot(acc && rank == need - 1);
            const int L = __ffsll((long long)cut) - 1;
            if (acc && rank < need) row[rank] = r;
            s += L + 1;
            k = 0;
            if (++d == nd) {
                done = true;
                end = s;
                break;
            }
            rng = rngs[d];
            mask = gen_mask(rng);
        }
        used += (unsigned long long)((done ? end : hi) - lo);
        if (!done) slice = slice == 2 ? 0 : slice + 1;
    }
    // numpy twists the whole key at once: bring the slices after the one the stream stopped in up to date
    if (slice == 0 || slice == 1)
        for (int q = slice + 1; q < 3; q++) twist_slice(key, SLICE_LO[q], SLICE_HI[q]);
    for (int i = lane; i < MT_N; i += 64) st->key[i] = key[i];
    if (lane == 0) {
        st->pos = (uint32_t)end;
        st->words += used;
    }
}

// Column totals (int64) and negative-count flags; a thread per column over a slab of genes, combined with atomics.
constexpr int TOT_SLAB = 512;
template <typename TIn>
__global__ __launch_bounds__(256) void ds_totals(const TIn *x, int64_t ldx, int G, int C, unsigned long long *tot, int *neg) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const int g0 = blockIdx.y * TOT_SLAB, g1 = min(G, g0 + TOT_SLAB);
    long long s = 0;
    bool n = false;
    for (int g = g0; g < g1; g++) {
        const long long v = (long long)x[(size_t)g * ldx + c];
        s += v;
        n |= v < 0;
    }
    atomicAdd(&tot[c], (unsigned long long)s);           // two's complement: the int64 sum
    if (n) atomicOr(&neg[c], 1);
}

// Columns that are not downsampled, unchanged (converted to the output type).
template <typename TIn, typename TOut>
__global__ __launch_bounds__(256) void ds_copy(const TIn *x, int64_t ldx, int G, int C, const int *is_ds, TOut *out, int64_t ldo) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C || is_ds[c]) return;
    for (int g = blockIdx.y; g < G; g += gridDim.y) out[(size_t)g * ldo + c] = (TOut)x[(size_t)g * ldx + c];
}

constexpr int HIST_CH = 2048, HIST_T = 256, HIST_PER = HIST_CH / HIST_T;

// One downsampled cell per workgroup: cells[d] is its column, rbuf[d * target ...] its accepted draws.
template <typename TIn, typename TOut>
__global__ __launch_bounds__(HIST_T) void ds_hist(const TIn *x, int64_t ldx, int G, const int *cells, const uint32_t *rbuf, int target,
                                                  TOut *out, int64_t ldo) {
    __shared__ long long cum[HIST_CH];
    __shared__ unsigned hist[HIST_CH];
    __shared__ long long part[HIST_T];
    const int t = threadIdx.x;
    const int c = cells[blockIdx.x];
    const uint32_t *r = rbuf + (size_t)blockIdx.x * target;
    long long base = 0;
    for (int g0 = 0; g0 < G; g0 += HIST_CH) {
        const int n = min(HIST_CH, G - g0);
        long long v[HIST_PER], s = 0;
#pragma unroll
        for (int j = 0; j < HIST_PER; j++) {
            const int gi = t * HIST_PER + j;
            s += gi < n ? (long long)x[(size_t)(g0 + gi) * ldx + c] : 0;
            v[j] = s;
        }
        part[t] = s;
        __syncthreads();
        for (int off = 1; off < HIST_T; off <<= 1) {          // inclusive scan of the per-thread sums
            const long long add = t >= off ? part[t - off] : 0;
            __syncthreads();
            part[t] += add;
            __syncthreads();
        }
        const long long excl = base + part[t] - s;
#pragma unroll
        for (int j = 0; j < HIST_PER; j++) {
            cum[t * HIST_PER + j] = excl + v[j];
            hist[t * HIST_PER + j] = 0;
        }
        const long long hi = base + part[HIST_T - 1];
        __syncthreads();
        for (int q = t; q < target; q += HIST_T) {
            const long long rv = r[q];
            if (rv < base || rv >= hi) continue;
            int a = 0, b = n - 1;                             // first gene of the chunk with cum > rv (exists: rv < hi)
            while (a < b) {
                const int m = (a + b) >> 1;
                if (cum[m] > rv) b = m; else a = m + 1;
            }
            atomicAdd(&hist[a], 1u);
        }
        __syncthreads();
        for (int gi = t; gi < n; gi += HIST_T) out[(size_t)(g0 + gi) * ldo + c] = (TOut)hist[gi];
        base = hi;
        __syncthreads();
    }
}

// Place-holder cells (cyto_placeholders), stage 2: the draws of a block of nk synthetic cells arrive cell-major from ds_stream,
// r[k * G + g] in [0, n), and select out[g][k0 + k] = own[g][r].  A 64 (genes) x 64 (cells) tile of r goes through LDS (rows
// padded to 65 words: the column read is conflict-free), so r is read along g and out is written along k; a wave's 64 gathers
// then fall into ONE row of own.  r == nullptr (n == 1): every cell is own's single column.  Tiles: blockIdx.x = kt * gtiles + gt.
constexpr int PH_TILE = 64, PH_T = 256;
template <typename TIn>
__global__ __launch_bounds__(PH_T) void ph_gather(const TIn *own, int64_t ld_own, int G, int n, const uint32_t *r, int nk, double *out,
                                                  int64_t ldo, int64_t k0, unsigned gtiles) {
    __shared__ uint32_t tile[PH_TILE][PH_TILE + 1];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int64_t gb = (int64_t)(blockIdx.x % gtiles) * PH_TILE;
    const int kb = (int)(blockIdx.x / gtiles) * PH_TILE;
    if (r) {
        const int64_t g = gb + tx;
        for (int kk = ty; kk < PH_TILE; kk += PH_T / 64) {
            const int k = kb + kk;
            if (k < nk && g < G) tile[kk][tx] = r[(size_t)k * (size_t)G + (size_t)g];
        }
        __syncthreads();
    }
    const int k = kb + tx;
    if (k >= nk) return;
    const uint32_t last = (uint32_t)(n - 1);
    for (int gg = ty; gg < PH_TILE; gg += PH_T / 64) {
        const int64_t g = gb + gg;
        if (g >= G) break;
        const uint32_t j = r ? min(tile[tx][gg], last) : 0u;         // (ds_stream accepts r <= n - 1 only)
        out[(size_t)g * (size_t)ldo + (size_t)(k0 + k)] = (double)own[(size_t)g * (size_t)ld_own + j];
    }
}

// (Mem, cyto_common.h: these buffers are as large as the count matrix and do not go through the block cache)

size_t dtype_size(int code) {
    switch (code) {
        case CYTO_DTYPE_U8: return 1;
        case CYTO_DTYPE_U16: return 2;
        case CYTO_DTYPE_I32: return 4;
        case CYTO_DTYPE_I64: return 8;
        default: return 0;
    }
}

template <typename TIn>
int launch_totals(const void *x, int64_t ldx, int G, int C, unsigned long long *tot, int *neg, hipStream_t s) {
    dim3 grid((unsigned)((C + 255) / 256), (unsigned)((G + TOT_SLAB - 1) / TOT_SLAB));
    hipLaunchKernelGGL(ds_totals<TIn>, grid, dim3(256), 0, s, (const TIn *)x, ldx, G, C, tot, neg);
    CYTO_HIP(hipGetLastError());
    return CYTO_OK;
}

template <typename TIn, typename TOut>
int launch_copy(const void *x, int64_t ldx, int G, int C, const int *is_ds, void *out, int64_t ldo, hipStream_t s) {
    dim3 grid((unsigned)((C + 255) / 256), (unsigned)std::min(G, 1024));
    hipLaunchKernelGGL((ds_copy<TIn, TOut>), grid, dim3(256), 0, s, (const TIn *)x, ldx, G, C, is_ds, (TOut *)out, ldo);
    CYTO_HIP(hipGetLastError());
    return CYTO_OK;
}

template <typename TIn, typename TOut>
int launch_hist(const void *x, int64_t ldx, int G, int nd, const int *cells, const uint32_t *rbuf, int target, void *out, int64_t ldo,
                hipStream_t s) {
    hipLaunchKernelGGL((ds_hist<TIn, TOut>), dim3((unsigned)nd), dim3(HIST_T), 0, s, (const TIn *)x, ldx, G, cells, rbuf, target,
                       (TOut *)out, ldo);
    CYTO_HIP(hipGetLastError());
    return CYTO_OK;
}

template <typename TOut>
int dispatch_in(int in_code, const void *x, int64_t ldx, int G, int C, const int *is_ds, void *out, int64_t ldo, hipStream_t s,
                int nd, const int *cells, const uint32_t *rbuf, int target, bool copy) {
    switch (in_code) {
        case CYTO_DTYPE_U8: return copy ? launch_copy<uint8_t, TOut>(x, ldx, G, C, is_ds, out, ldo, s)
                                        : launch_hist<uint8_t, TOut>(x, ldx, G, nd, cells, rbuf, target, out, ldo, s);
        case CYTO_DTYPE_U16: return copy ? launch_copy<uint16_t, TOut>(x, ldx, G, C, is_ds, out, ldo, s)
                                         : launch_hist<uint16_t, TOut>(x, ldx, G, nd, cells, rbuf, target, out, ldo, s);
        case CYTO_DTYPE_I32: return copy ? launch_copy<int32_t, TOut>(x, ldx, G, C, is_ds, out, ldo, s)
                                         : launch_hist<int32_t, TOut>(x, ldx, G, nd, cells, rbuf, target, out, ldo, s);
        default: return copy ? launch_copy<int64_t, TOut>(x, ldx, G, C, is_ds, out, ldo, s)
                             : launch_hist<int64_t, TOut>(x, ldx, G, nd, cells, rbuf, target, out, ldo, s);
    }
}

int dispatch(int in_code, int out_code, const void *x, int64_t ldx, int G, int C, const int *is_ds, void *out, int64_t ldo,
             hipStream_t s, int nd, const int *cells, const uint32_t *rbuf, int target, bool copy) {
    if (out_code == CYTO_DTYPE_U16)
        return dispatch_in<uint16_t>(in_code, x, ldx, G, C, is_ds, out, ldo, s, nd, cells, rbuf, target, copy);
    return dispatch_in<int64_t>(in_code, x, ldx, G, C, is_ds, out, ldo, s, nd, cells, rbuf, target, copy);
}

template <typename TIn>
int launch_gather(const void *own, int64_t ld_own, int G, int n, const uint32_t *r, int nk, double *out, int64_t ldo, int64_t k0,
                  hipStream_t s) {
    const unsigned gtiles = (unsigned)((G + PH_TILE - 1) / PH_TILE), ktiles = (unsigned)((nk + PH_TILE - 1) / PH_TILE);
    hipLaunchKernelGGL(ph_gather<TIn>, dim3(gtiles * ktiles), dim3(PH_T), 0, s, (const TIn *)own, ld_own, G, n, r, nk, out, ldo, k0,
                       gtiles);
    CYTO_HIP(hipGetLastError());
    return CYTO_OK;
}

int dispatch_gather(int code, const void *own, int64_t ld_own, int G, int n, const uint32_t *r, int nk, double *out, int64_t ldo,
                    int64_t k0, hipStream_t s) {
    switch (code) {
        case CYTO_DTYPE_U16: return launch_gather<uint16_t>(own, ld_own, G, n, r, nk, out, ldo, k0, s);
        case CYTO_DTYPE_F64: return launch_gather<double>(own, ld_own, G, n, r, nk, out, ldo, k0, s);
        default: return launch_gather<int64_t>(own, ld_own, G, n, r, nk, out, ldo, k0, s);
    }
}

// accepted draws of one block of cells: 1 GiB (CYTO_DS_RBUF_BYTES: smaller blocks, for tests of the block hand-over)
size_t rbuf_bytes() {
    const Knob &k = CYTO_KNOB("CYTO_DS_RBUF_BYTES");
    return k.set && k.value > 0 ? (size_t)k.value : size_t(1) << 30;
}

int load_state(MtState &h, const uint32_t *key, const int32_t *pos) {
    if (*pos < 0 || *pos > MT_N) return CYTO_ERR_BAD_ARG;
    memcpy(h.key, key, sizeof h.key);
    h.pos = (uint32_t)*pos;
    h.pad = 0;
    h.words = 0;
    return CYTO_OK;
}

}  // namespace

namespace {
// cyto_downsample (on_device = false: x and out are host matrices, staged through dx / dout) and cyto_downsample_dev (true: the
// kernels read x and write out where they lie, with the caller's leading dimensions)
int downsample_impl(int G, int C, const void *x, int64_t ldx, int x_dtype, void *out, int64_t ldo, int out_dtype, int target,
                    uint32_t *key, int32_t *pos, int64_t *words_out, int device_id, bool on_device) {
    if (G <= 0 || C <= 0 || !x || !out || ldx < C || ldo < C || target < 0 || !key || !pos) return CYTO_ERR_BAD_ARG;
    const size_t in_sz = dtype_size(x_dtype);
    if (!in_sz || (out_dtype != CYTO_DTYPE_I64 && out_dtype != CYTO_DTYPE_U16)) return CYTO_ERR_BAD_ARG;
    if (out_dtype == CYTO_DTYPE_U16 && target > 65535) return CYTO_ERR_BAD_ARG;
    MtState hs;
    int rc = load_state(hs, key, pos);
    if (rc) return rc;
    if ((rc = select_device(device_id))) return rc;
    const size_t out_sz = out_dtype == CYTO_DTYPE_U16 ? 2 : 8;
    std::vector<int64_t> tot(C);
    std::vector<int> neg(C), flag(C), cells;
    std::vector<uint32_t> rngs;
    // (declared before the streams: the streams drain before any buffer is freed, whatever path leaves the call)
    Mem dx, dout, dtot, dneg, dflag, dstate, dcells, drng, drbuf;
    StreamGuard sa, sb;                                  // sa: upload, totals, copies, stage 2; sb: stage 1
    if ((rc = sa.acquire()) || (rc = sb.acquire())) return rc;
    if ((rc = dtot.alloc((size_t)C * 8)) || (rc = dneg.alloc((size_t)C * 4)) || (rc = dflag.alloc((size_t)C * 4)) ||
        (rc = dstate.alloc(sizeof(MtState))))
        return rc;
    if (!on_device) {
        if ((rc = dx.alloc((size_t)G * C * in_sz)) || (rc = dout.alloc((size_t)G * C * out_sz))) return rc;
        CYTO_HIP(hipMemcpy2DAsync(dx.p, (size_t)C * in_sz, x, (size_t)ldx * in_sz, (size_t)C * in_sz, (size_t)G, hipMemcpyHostToDevice, sa.s));
    }
    const void *xp = on_device ? x : dx.p;                // the matrices as the kernels see them
    void *op = on_device ? out : dout.p;
    const int64_t xl = on_device ? ldx : C, ol = on_device ? ldo : C;
    CYTO_HIP(hipMemsetAsync(dtot.p, 0, (size_t)C * 8, sa.s));
    CYTO_HIP(hipMemsetAsync(dneg.p, 0, (size_t)C * 4, sa.s));
    switch (x_dtype) {
        case CYTO_DTYPE_U8: rc = launch_totals<uint8_t>(xp, xl, G, C, dtot.as<unsigned long long>(), dneg.as<int>(), sa.s); break;
        case CYTO_DTYPE_U16: rc = launch_totals<uint16_t>(xp, xl, G, C, dtot.as<unsigned long long>(), dneg.as<int>(), sa.s); break;
        case CYTO_DTYPE_I32: rc = launch_totals<int32_t>(xp, xl, G, C, dtot.as<unsigned long long>(), dneg.as<int>(), sa.s); break;
        default: rc = launch_totals<int64_t>(xp, xl, G, C, dtot.as<unsigned long long>(), dneg.as<int>(), sa.s); break;
    }
    if (rc) return rc;
    CYTO_HIP(hipMemcpyAsync(tot.data(), dtot.p, (size_t)C * 8, hipMemcpyDeviceToHost, sa.s));
    CYTO_HIP(hipMemcpyAsync(neg.data(), dneg.p, (size_t)C * 4, hipMemcpyDeviceToHost, sa.s));
    CYTO_HIP(hipStreamSynchronize(sa.s));

    // the downsampled cells, in column order; what np.repeat / randint would refuse is refused before any word is drawn
    bool any_neg = false;
    for (int c = 0; c < C; c++) {
        any_neg |= neg[c] != 0;
        flag[c] = tot[c] > (int64_t)target;
        if (!flag[c]) continue;
        if (neg[c]) return CYTO_ERR_BAD_ARG;                                   // np.repeat: negative count
        if (target > 0 && tot[c] > (int64_t(1) << 32)) return CYTO_ERR_BAD_ARG; // numpy switches to 64-bit draws
        cells.push_back(c);
        rngs.push_back((uint32_t)(tot[c] - 1));
    }
    if (any_neg && out_dtype == CYTO_DTYPE_U16) return CYTO_ERR_BAD_ARG;       // a kept negative count has no uint16 value
    const int nd = (int)cells.size();
    CYTO_HIP(hipMemcpyAsync(dflag.p, flag.data(), (size_t)C * 4, hipMemcpyHostToDevice, sa.s));
    if ((rc = dispatch(x_dtype, out_dtype, xp, xl, G, C, dflag.as<int>(), op, ol, sa.s, 0, nullptr, nullptr, 0, true))) return rc;

    if (nd > 0) {
        const int per = (int)std::max<size_t>(1, std::min<size_t>((size_t)nd, target ? rbuf_bytes() / ((size_t)target * 4) : (size_t)nd));
        const int nblocks = (nd + per - 1) / per;
        if ((rc = dcells.alloc((size_t)nd * 4)) || (rc = drng.alloc((size_t)nd * 4)) ||
            (rc = drbuf.alloc((size_t)std::min(nblocks, 2) * per * (size_t)target * 4)))
            return rc;
        CYTO_HIP(hipMemcpyAsync(dcells.p, cells.data(), (size_t)nd * 4, hipMemcpyHostToDevice, sa.s));
        CYTO_HIP(hipMemcpyAsync(drng.p, rngs.data(), (size_t)nd * 4, hipMemcpyHostToDevice, sa.s));
        CYTO_HIP(hipMemcpyAsync(dstate.p, &hs, sizeof hs, hipMemcpyHostToDevice, sa.s));
        Events<5> ev;                                   // 0: inputs ready; 1,2: stage 1 of buffer 0/1 done; 3,4: stage 2 of it done
        if ((rc = ev.create())) return rc;
        CYTO_HIP(hipEventRecord(ev[0], sa.s));
        CYTO_HIP(hipStreamWaitEvent(sb.s, ev[0], 0));
        for (int b = 0; b < nblocks; b++) {
            const int d0 = b * per, n = std::min(per, nd - d0), buf = b & 1;
            uint32_t *rb = drbuf.as<uint32_t>() + (size_t)buf * per * target;
            if (b >= 2) CYTO_HIP(hipStreamWaitEvent(sb.s, ev[3 + buf], 0));
            if (target > 0) {
                hipLaunchKernelGGL(ds_stream, dim3(1), dim3(64), 0, sb.s, dstate.as<MtState>(), drng.as<uint32_t>() + d0, n, target, rb);
                CYTO_HIP(hipGetLastError());
            }
            CYTO_HIP(hipEventRecord(ev[1 + buf], sb.s));
            CYTO_HIP(hipStreamWaitEvent(sa.s, ev[1 + buf], 0));
            if ((rc = dispatch(x_dtype, out_dtype, xp, xl, G, C, nullptr, op, ol, sa.s, n, dcells.as<int>() + d0, rb, target, false)))
                return rc;
            CYTO_HIP(hipEventRecord(ev[3 + buf], sa.s));
        }
        CYTO_HIP(hipStreamSynchronize(sb.s));
        CYTO_HIP(hipMemcpyAsync(&hs, dstate.p, sizeof hs, hipMemcpyDeviceToHost, sa.s));
    }
    if (!on_device)
        CYTO_HIP(hipMemcpy2DAsync(out, (size_t)ldo * out_sz, dout.p, (size_t)C * out_sz, (size_t)C * out_sz, (size_t)G, hipMemcpyDeviceToHost,
                                  sa.s));
    CYTO_HIP(hipStreamSynchronize(sa.s));
    memcpy(key, hs.key, sizeof hs.key);
    *pos = (int32_t)hs.pos;
    if (words_out) *words_out = (int64_t)hs.words;
    return CYTO_OK;
}
}  // namespace

int cyto_downsample(int G, int C, const void *x, int64_t ldx, int x_dtype, void *out, int64_t ldo, int out_dtype, int target,
                    uint32_t *key, int32_t *pos, int64_t *words_out, int device_id) {
    return downsample_impl(G, C, x, ldx, x_dtype, out, ldo, out_dtype, target, key, pos, words_out, device_id, false);
}

int cyto_downsample_dev(int G, int C, const void *x_dev, int64_t ldx, int x_dtype, void *out_dev, int64_t ldo, int out_dtype, int target,
                        uint32_t *key, int32_t *pos, int64_t *words_out, int device_id) {
    if (x_dev == out_dev) return CYTO_ERR_BAD_ARG;
    return downsample_impl(G, C, x_dev, ldx, x_dtype, out_dev, ldo, out_dtype, target, key, pos, words_out, device_id, true);
}

int cyto_placeholders(int G, int n, const void *own, int64_t ld_own, int own_dtype, int64_t short_count, double *out, int64_t ldo,
                      uint32_t *key, int32_t *pos, int64_t *words_out, int64_t cap_bytes, int device_id) {
    if (G <= 0 || n <= 0 || short_count < 0 || !own || !out || !key || !pos || ld_own < n || ldo < short_count || cap_bytes < 0)
        return CYTO_ERR_BAD_ARG;
    const size_t in_sz = own_dtype == CYTO_DTYPE_U16 ? 2 : own_dtype == CYTO_DTYPE_I64 || own_dtype == CYTO_DTYPE_F64 ? 8 : 0;
    if (!in_sz) return CYTO_ERR_BAD_ARG;
    MtState hs;
    int rc = load_state(hs, key, pos);
    if (rc) return rc;
    if (words_out) *words_out = 0;
    if (short_count == 0) return CYTO_OK;
    if ((rc = select_device(device_id))) return rc;
    // a block's draws: at most the cap (never above the default, which also bounds a launch's tiles), at least one cell
    const size_t cap = cap_bytes ? std::min((size_t)cap_bytes, rbuf_bytes()) : rbuf_bytes();
    const int64_t per = std::max<int64_t>(1, std::min<int64_t>(short_count, (int64_t)(cap / ((size_t)G * 4))));
    const int64_t nblocks = (short_count + per - 1) / per;
    const bool draw = n > 1;                             // randint(0, 1) takes no word
    Mem down, dout, dstate, drng, drbuf;                 // (declared before the streams, as in cyto_downsample)
    StreamGuard sa, sb;                                  // sa: upload, stage 2, download; sb: stage 1
    if ((rc = sa.acquire()) || (rc = sb.acquire())) return rc;
    if ((rc = down.alloc((size_t)G * n * in_sz)) || (rc = dout.alloc((size_t)G * (size_t)short_count * 8))) return rc;
    CYTO_HIP(hipMemcpy2DAsync(down.p, (size_t)n * in_sz, own, (size_t)ld_own * in_sz, (size_t)n * in_sz, (size_t)G, hipMemcpyHostToDevice,
                              sa.s));
    if (!draw) {
        for (int64_t b = 0; b < nblocks; b++) {
            const int64_t k0 = b * per;
            if ((rc = dispatch_gather(own_dtype, down.p, n, G, n, nullptr, (int)std::min(per, short_count - k0), dout.as<double>(),
                                      short_count, k0, sa.s)))
                return rc;
        }
    } else {
        if ((rc = dstate.alloc(sizeof(MtState))) || (rc = drng.alloc((size_t)per * 4)) ||
            (rc = drbuf.alloc((size_t)std::min<int64_t>(nblocks, 2) * (size_t)per * (size_t)G * 4)))
            return rc;
        CYTO_HIP(hipMemsetD32Async((hipDeviceptr_t)drng.p, n - 1, (size_t)per, sa.s));       // every synthetic cell draws below n
        CYTO_HIP(hipMemcpyAsync(dstate.p, &hs, sizeof hs, hipMemcpyHostToDevice, sa.s));
        Events<5> ev;                                   // 0: inputs ready; 1,2: stage 1 of buffer 0/1 done; 3,4: stage 2 of it done
        if ((rc = ev.create())) return rc;
        CYTO_HIP(hipEventRecord(ev[0], sa.s));
        CYTO_HIP(hipStreamWaitEvent(sb.s, ev[0], 0));
        for (int64_t b = 0; b < nblocks; b++) {
            const int64_t k0 = b * per;
            const int nk = (int)std::min(per, short_count - k0), buf = (int)(b & 1);
            uint32_t *rb = drbuf.as<uint32_t>() + (size_t)buf * (size_t)per * (size_t)G;
            if (b >= 2) CYTO_HIP(hipStreamWaitEvent(sb.s, ev[3 + buf], 0));
            hipLaunchKernelGGL(ds_stream, dim3(1), dim3(64), 0, sb.s, dstate.as<MtState>(), drng.as<uint32_t>(), nk, G, rb);
            CYTO_HIP(hipGetLastError());
            CYTO_HIP(hipEventRecord(ev[1 + buf], sb.s));
            CYTO_HIP(hipStreamWaitEvent(sa.s, ev[1 + buf], 0));
            if ((rc = dispatch_gather(own_dtype, down.p, n, G, n, rb, nk, dout.as<double>(), short_count, k0, sa.s))) return rc;
            CYTO_HIP(hipEventRecord(ev[3 + buf], sa.s));
        }
        CYTO_HIP(hipStreamSynchronize(sb.s));
        CYTO_HIP(hipMemcpyAsync(&hs, dstate.p, sizeof hs, hipMemcpyDeviceToHost, sa.s));
    }
    CYTO_HIP(hipMemcpy2DAsync(out, (size_t)ldo * 8, dout.p, (size_t)short_count * 8, (size_t)short_count * 8, (size_t)G,
                              hipMemcpyDeviceToHost, sa.s));
    CYTO_HIP(hipStreamSynchronize(sa.s));
    memcpy(key, hs.key, sizeof hs.key);
    *pos = (int32_t)hs.pos;
    if (words_out) *words_out = (int64_t)hs.words;
    return CYTO_OK;
}

int cyto_mt19937_fill(uint32_t *key, int32_t *pos, int n, uint32_t *words, int device_id) {
    if (!key || !pos || n < 0 || (n > 0 && !words)) return CYTO_ERR_BAD_ARG;
    MtState hs;
    int rc = load_state(hs, key, pos);
    if (rc) return rc;
    if (n == 0) return CYTO_OK;
    if ((rc = select_device(device_id))) return rc;
    Mem dstate, drng, dw;
    StreamGuard sg;
    if ((rc = sg.acquire())) return rc;
    if ((rc = dstate.alloc(sizeof(MtState))) || (rc = drng.alloc(4)) || (rc = dw.alloc((size_t)n * 4))) return rc;
    const uint32_t all = 0xffffffffu;                   // T = 2^32: every raw word is accepted as it is
    CYTO_HIP(hipMemcpyAsync(dstate.p, &hs, sizeof hs, hipMemcpyHostToDevice, sg.s));
    CYTO_HIP(hipMemcpyAsync(drng.p, &all, 4, hipMemcpyHostToDevice, sg.s));
    hipLaunchKernelGGL(ds_stream, dim3(1), dim3(64), 0, sg.s, dstate.as<MtState>(), drng.as<uint32_t>(), 1, n, dw.as<uint32_t>());
    CYTO_HIP(hipGetLastError());
    CYTO_HIP(hipMemcpyAsync(words, dw.p, (size_t)n * 4, hipMemcpyDeviceToHost, sg.s));
    CYTO_HIP(hipMemcpyAsync(&hs, dstate.p, sizeof hs, hipMemcpyDeviceToHost, sg.s));
    CYTO_HIP(hipStreamSynchronize(sg.s));
    memcpy(key, hs.key, sizeof hs.key);
    *pos = (int32_t)hs.pos;
    return CYTO_OK;
}
