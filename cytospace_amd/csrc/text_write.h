// text_write.h -- what the two device text writers (mtx.hip: MatrixMarket, csv.hip: the place-holder table) share: the decimal digit
// routines, which host and device both compile, the workgroup scan of their count and format passes, and the host's output file.
#pragma once
#include "cyto_common.h"

#include <errno.h>
#include <unistd.h>

#include <chrono>

namespace cyto {

__host__ __device__ inline int ndigits32(uint32_t v) {
    return v < 10u ? 1 : v < 100u ? 2 : v < 1000u ? 3 : v < 10000u ? 4 : v < 100000u ? 5 : v < 1000000u ? 6 : v < 10000000u ? 7
         : v < 100000000u ? 8 : v < 1000000000u ? 9 : 10;
}

__host__ __device__ inline int ndigits64(uint64_t v) {
    if (v <= 0xffffffffull) return ndigits32((uint32_t)v);
    int n = 10;
    for (uint64_t p = 10000000000ull; n < 20 && v >= p; p *= 10) n++;   // (p wraps only after n has reached 20)
    return n;
}

// o[0, nd) := the nd decimal digits of v (nd = ndigits64(v)); 32-bit arithmetic once what is left fits.
__host__ __device__ inline void put_digits(uint8_t *o, uint64_t v, int nd) {
    int i = nd;
    while (v > 0xffffffffull) {
        const uint64_t q = v / 1000000000ull;
        uint32_t r = (uint32_t)(v - q * 1000000000ull);
        for (int k = 0; k < 9; k++) {
            o[--i] = (uint8_t)('0' + r % 10u);
            r /= 10u;
        }
        v = q;
    }
    uint32_t w = (uint32_t)v;
    while (i > 0) {
        o[--i] = (uint8_t)('0' + w % 10u);
        w /= 10u;
    }
}

// Exclusive scan of one value per thread across a workgroup of NT threads; *total: the sum.  Every thread must call it.
template <int NT, typename V> __device__ __forceinline__ V wg_scan(V v, V *total) {
    __shared__ V wsum[NT / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    V x = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const V y = __shfl_up(x, off, 64);
        if (lane >= off) x += y;
    }
    if (lane == 63) wsum[w] = x;
    __syncthreads();
    V before = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < NT / 64; i++) {
        before += i < w ? wsum[i] : V(0);
        tot += wsum[i];
    }
    __syncthreads();                                    // (wsum is reused by the next call)
    *total = tot;
    return before + x - v;
}

// The output file: removed again unless the whole of it was written.
struct OutFile {
    int fd = -1;
    const char *path = nullptr;
    bool keep = false;
    ~OutFile() {
        if (fd < 0) return;
        close(fd);
        if (!keep) unlink(path);
    }
    bool write_all(const void *buf, size_t n) {
        const char *q = static_cast<const char *>(buf);
        while (n > 0) {
            const ssize_t r = write(fd, q, n);
            if (r < 0 && errno == EINTR) continue;
            if (r <= 0) return false;
            q += r;
            n -= (size_t)r;
        }
        return true;
    }
};

inline double ms_since(std::chrono::steady_clock::time_point t) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
}

inline size_t dtype_size(int dt) {
    switch (dt) {
    case CYTO_DTYPE_U8: return 1;
    case CYTO_DTYPE_U16: return 2;
    case CYTO_DTYPE_F32: case CYTO_DTYPE_I32: return 4;
    case CYTO_DTYPE_F64: case CYTO_DTYPE_I64: return 8;
    }
    return 0;
}

}  // namespace cyto
