// select_exact.h -- "does this value survive the conversion" for cyto_select, for host and device from one function (the host hook
// cyto_select_check and the kernels of resident.hip include it, as mtx.hip and csv.hip share shortest.h).
//
// converts_exactly<TD>(v) is numpy's round trip  v.astype(dst).astype(src) == v  without its undefined corners: a NaN never
// survives (NaN != NaN, the identity conversion included), an infinity survives a conversion to float32 / float64 only, -0.0
// survives every conversion (it compares equal to the 0 it becomes), and a value outside the destination's range does not.
// convert_value<TD>(v) is the plain cast to float32 / float64 (every value has one: a same-type "conversion" copies the bits, NaN
// included) and, to an integer type, the plain cast for a value that survives and 0 for one that does not (a float-to-integer cast
// out of range is undefined in C++; cyto_select leaves such elements unspecified).
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace cyto {

template <typename T> struct is_float_type { static constexpr bool value = false; };
template <> struct is_float_type<float> { static constexpr bool value = true; };
template <> struct is_float_type<double> { static constexpr bool value = true; };

// a float32 / float64 value is an integer within [lo, hi] (both exactly representable in F)
template <typename F> __host__ __device__ inline bool integral_in(F v, F lo, F hi) {
    return v >= lo && v <= hi && (F)(long long)v == v;       // (false for a NaN; |v| <= 2^63 is checked by the callers' bounds)
}

template <typename TD, typename TS> __host__ __device__ inline bool converts_exactly(TS v) {
    if constexpr (is_float_type<TS>::value) {
        if (v != v) return false;
        if constexpr (sizeof(TD) == 1) return integral_in<TS>(v, (TS)0, (TS)255);
        else if constexpr (sizeof(TD) == 2) return integral_in<TS>(v, (TS)0, (TS)65535);
        else if constexpr (!is_float_type<TD>::value)        // int64: [-2^63, 2^63), the upper bound as the largest value below it
            return integral_in<TS>(v, (TS)-9223372036854775808.0, sizeof(TS) == 4 ? (TS)9223371487098961920.0 : (TS)9223372036854774784.0);
        else if constexpr (sizeof(TD) < sizeof(TS)) {        // float64 -> float32
            if (v - v != 0) return true;                     // an infinity
            if (v > 3.4028234663852886e38 || v < -3.4028234663852886e38) return false;
            return (TS)(TD)v == v;
        } else
            return true;
    } else if constexpr (sizeof(TS) == 2) {                  // uint16
        if constexpr (sizeof(TD) == 1) return v <= 255;
        else return true;
    } else {                                                 // int64
        if constexpr (sizeof(TD) == 1) return v >= 0 && v <= 255;
        else if constexpr (sizeof(TD) == 2) return v >= 0 && v <= 65535;
        else if constexpr (!is_float_type<TD>::value) return true;
        else {
            const TD f = (TD)v;                              // round to nearest; 2^63 for the values that round up to it
            return f < (TD)9223372036854775808.0 && (int64_t)f == v;
        }
    }
}

template <typename TD, typename TS> __host__ __device__ inline TD convert_value(TS v) {
    if constexpr (is_float_type<TD>::value) return (TD)v;    // (always defined: the rounded value, a NaN stays one)
    else return converts_exactly<TD, TS>(v) ? (TD)v : (TD)0;
}

}  // namespace cyto
