// hz_q16.h -- the 16-bit horizon code (clause 15): a horizon angle in [-pi/2, pi/2] as one of 65535
// equally spaced levels, 0xFFFF for NaN.  All arithmetic is float64 and every operation is rounded on its own (the library is
// built with -ffp-contract=off); rint rounds half to even.  The look-up kernels read a horizon of either element type
// through hori_value(): a code is decoded to float32 first and that float32 is widened, so a handle on codes q answers with
// the words of a handle on the float32 array decode(q).
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

namespace hz {

#define HZ_Q16_NAN 0xFFFFu
#define HZ_Q16_HALF_PI 1.5707963267948966
#define HZ_Q16_SCALE (32767.0 / HZ_Q16_HALF_PI)
#define HZ_Q16_STEP (HZ_Q16_HALF_PI / 32767.0)

// NaN -> 0xFFFF; everything else, +-inf included, clamps to the range first: 0 ... 65534, +-0 -> 32767
__host__ __device__ __forceinline__ uint16_t q16_encode(float v) {
    if (v != v) return (uint16_t)HZ_Q16_NAN;
    const double c = fmin(fmax((double)v, -HZ_Q16_HALF_PI), HZ_Q16_HALF_PI);
    return (uint16_t)(rint(c * HZ_Q16_SCALE) + 32767.0);
}

// 0xFFFF -> the quiet NaN 0x7FC00000; 32767 -> +0.0f
__host__ __device__ __forceinline__ float q16_decode(uint16_t q) {
    if (q == (uint16_t)HZ_Q16_NAN) return __builtin_nanf("");
    return (float)((double)((int)q - 32767) * HZ_Q16_STEP);
}

// one horizon element as the float64 the look-up continues with
__device__ __forceinline__ double hori_value(float v) { return (double)v; }
__device__ __forceinline__ double hori_value(uint16_t q) { return (double)q16_decode(q); }

}  // namespace hz
