// hz_crmath_probe.hip -- test hooks that evaluate the refraction math on the device, element by element.
//
// hz_crmath.h and hz_horisun_refrac.h are compiled twice: by gcc into the CPU oracle and by hipcc into the kernels.  The two
// compiles are different programs (the device's float64 sqrt and division are instruction sequences the compiler writes), so
// "both include the same header" proves nothing about the words.  This file is the device compile on its own, behind
// hz_debug_crmath_eval / hz_debug_crmath_range / hz_debug_refrac_factor; tests/test_gpu_crmath.py holds it word for word to
// the oracle's compile (orc_crmath_eval / orc_crmath_range) and to the mpmath fixture tests/golden/crmath_reference.npz.
// Built with the library's flags like every other file: what the probe evaluates is what the kernels evaluate.
#include "hz_internal.h"
#include "hz_horisun_refrac.h"

namespace hz {

#define CRM_PROBE_FUNCS 8

// which: 0 acos, 1 tan, 2 cos, 3 sin, 4 pow(x, y), 5 deg2rad, 6 rad2deg, 7 atmos_refrac(x, (double)y)
__device__ __forceinline__ float crmath_probe_one(int which, float x, float y) {
    switch (which) {
        case 0: return hz_crm_acosf(x);
        case 1: return hz_crm_tanf(x);
        case 2: return hz_crm_cosf(x);
        case 3: return hz_crm_sinf(x);
        case 4: return hz_crm_powf(x, y);
        case 5: return horisun_deg2rad_f(x);
        case 6: return horisun_rad2deg_f(x);
        default: return horisun_atmos_refrac(x, (double)y);
    }
}

// One thread per element.  x null: element i is the float with the bit pattern first_bits + i * stride (uint32 arithmetic).
// y null: every element takes y_all.
__global__ __launch_bounds__(256) void k_crmath_probe(int which, const float *__restrict__ x, const float *__restrict__ y,
                                                      uint32_t first_bits, uint32_t stride, float y_all, size_t n,
                                                      float *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float xi = x ? x[i] : __uint_as_float(first_bits + (uint32_t)i * stride);
    const float yi = y ? y[i] : y_all;
    out[i] = crmath_probe_one(which, xi, yi);
}

// host x / y (either may be null, see the kernel) -> host out
static int crmath_probe_run(int which, const float *x, const float *y, uint32_t first_bits, uint32_t stride, float y_all,
                            size_t n, float *out, int device) {
    if (which < 0 || which >= CRM_PROBE_FUNCS) return set_error(HZ_ERR_ARG, "crmath probe: function %d out of range", which);
    if (n > 0x7fffffffull) return set_error(HZ_ERR_ARG, "crmath probe: too many elements");
    if (n == 0) return HZ_OK;
    if (!out) return set_error(HZ_ERR_ARG, "NULL argument");
    int rc = select_device(device);
    if (rc) return rc;
    hipStream_t st = nullptr;
    DevBuf dx, dy, dout;
    HZ_HIP(dout.alloc(n * 4));
    if (x) { HZ_HIP(dx.alloc(n * 4)); HZ_HIP(hipMemcpy(dx.p, x, n * 4, hipMemcpyHostToDevice)); }
    if (y) { HZ_HIP(dy.alloc(n * 4)); HZ_HIP(hipMemcpy(dy.p, y, n * 4, hipMemcpyHostToDevice)); }
    hipLaunchKernelGGL(k_crmath_probe, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, which, (const float *)dx.p,
                       (const float *)dy.p, first_bits, stride, y_all, n, (float *)dout.p);
    HZ_HIP(hipGetLastError());
    HZ_HIP(hipStreamSynchronize(st));
    HZ_HIP(hipMemcpy(out, dout.p, n * 4, hipMemcpyDeviceToHost));
    return HZ_OK;
}

}  // namespace hz

using namespace hz;

extern "C" {

int hz_debug_crmath_eval(int which, const float *x, const float *y, float *out, size_t n, int device) {
    if (n && !x) return set_error(HZ_ERR_ARG, "NULL argument");
    return crmath_probe_run(which, x, y, 0u, 0u, 0.0f, n, out, device);
}

int hz_debug_crmath_range(int which, uint32_t first_bits, uint32_t stride, size_t n, float y, float *out, int device) {
    return crmath_probe_run(which, nullptr, nullptr, first_bits, stride, y, n, out, device);
}

int hz_debug_refrac_factor(const float *elevation, size_t n, double *out_f64, int device) {
    if (n == 0) return HZ_OK;
    if (!elevation || !out_f64) return set_error(HZ_ERR_ARG, "NULL argument");
    if (n > 0x7fffffffull) return set_error(HZ_ERR_ARG, "crmath probe: too many elements");
    int rc = select_device(device);
    if (rc) return rc;
    hipStream_t st = nullptr;
    DevBuf delev, dout;
    HZ_HIP(delev.alloc(n * 4)); HZ_HIP(dout.alloc(n * 8));
    HZ_HIP(hipMemcpy(delev.p, elevation, n * 4, hipMemcpyHostToDevice));
    if ((rc = shadow_refrac_factor((const float *)delev.p, n, (double *)dout.p, st))) return rc;
    HZ_HIP(hipStreamSynchronize(st));
    HZ_HIP(hipMemcpy(out_f64, dout.p, n * 8, hipMemcpyDeviceToHost));
    return HZ_OK;
}

}  // extern "C"
