// text_scan.h -- what the two text readers (table.hip, mtx_read.hip) share: the workgroup scan, the 64 KiB block geometry of the
// line-end pass, the scan of the block counts, the lowest-byte refusal word, and the host pieces of the chunked upload.
#pragma once
#include "cyto_common.h"

#include <unistd.h>

#include <chrono>

namespace {

// The refusal with the lowest byte offset wins, whatever the launch order: *err := min(*err, pos << 8 | kind).
__device__ __forceinline__ void note_error(unsigned long long *err, int64_t pos, int kind) {
    atomicMin(err, ((unsigned long long)pos << 8) | (unsigned long long)kind);
}

constexpr int WG = 256;

// Exclusive scan of one value per thread across the 256-thread workgroup; *total: the sum.  Every thread must call it.
__device__ __forceinline__ int wg_scan(int v, int *total) {
    __shared__ int wsum[WG / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int y = __shfl_up(x, off, 64);
        if (lane >= off) x += y;
    }
    if (lane == 63) wsum[w] = x;
    __syncthreads();
    int before = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < WG / 64; i++) {
        before += i < w ? wsum[i] : 0;
        tot += wsum[i];
    }
    __syncthreads();                                    // (wsum is reused by the next call)
    *total = tot;
    return before + x - v;
}

// A thread owns 16 consecutive 16-byte slices (256 bytes), a workgroup 64 KiB.
constexpr int NL_SLICES = 16;
constexpr int64_t NL_BLOCK = (int64_t)WG * NL_SLICES * 16;

__device__ __forceinline__ uint8_t byte_of(const uint4 &v, int k) {
    const uint32_t w = k < 4 ? v.x : k < 8 ? v.y : k < 12 ? v.z : v.w;
    return (uint8_t)(w >> ((k & 3) * 8));
}

// One workgroup: off[b] := exclusive prefix sum of cnt over the nblk blocks, *total := the sum.
__global__ __launch_bounds__(WG) void tbl_scan_blocks(const int *cnt, int64_t nblk, int64_t *off, int64_t *total) {
    int64_t carry = 0;
    for (int64_t b0 = 0; b0 < nblk; b0 += WG) {
        const int64_t b = b0 + threadIdx.x;
        const int v = b < nblk ? cnt[b] : 0;
        int tot;
        const int ex = wg_scan(v, &tot);
        if (b < nblk) off[b] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) *total = carry;
}

// (the streamed upload: the file is read in chunks into two pinned buffers, cyto_common.h: Pinned)
constexpr size_t CHUNK = size_t(16) << 20;

struct Fd {
    int fd = -1;
    ~Fd() { if (fd >= 0) close(fd); }
};

[[maybe_unused]] double ms_since(std::chrono::steady_clock::time_point t) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
}

}  // namespace
