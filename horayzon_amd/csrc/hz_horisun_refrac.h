// hz_horisun_refrac.h -- atmospheric refraction for the look-up kernels of HorizonTerrain (k_horisun, k_horisun_planes,
// k_horisun_coarse; DESIGN.md section 4, clause 13).
//
// The refraction branch of shadow_setup (hz_shadow.hip, `p.refrac == 1`; shadow_comp.cpp:430-446) written again in the same
// order of operations, as horisun_unit restates vec_unit: that file's text and machine code do not move.  The five float libm
// calls are the correctly rounded floats of hz_crmath.h and every user is built with -ffp-contract=off, so the bent direction
// and the two dot products are the words Terrain(refrac_cor=True) forms for the same cell.
#ifndef HZ_HORISUN_REFRAC_H
#define HZ_HORISUN_REFRAC_H

#include "hz_crmath.h"

namespace hz {

// shadow_comp.cpp:43-62: float in, double arithmetic, float out (deg2rad_f / rad2deg_f of hz_shadow.hip)
__device__ __forceinline__ float horisun_deg2rad_f(float a) {
    return (float)(hz_crm_div_const((double)a, 180.0, 1.0 / 180.0) * 3.14159265358979323846);
}
__device__ __forceinline__ float horisun_rad2deg_f(float a) {
    return (float)(hz_crm_div_const((double)a, 3.14159265358979323846, 1.0 / 3.14159265358979323846) * 180.0);
}

// shadow_comp.cpp:96-106 (vec_unit of hz_shadow.hip)
__device__ __forceinline__ void horisun_refrac_unit(float &x, float &y, float &z) {
    const float mag = __builtin_sqrtf((x * x + y * y) + z * z);
    x = x / mag; y = y / mag; z = z / mag;
}

// shadow_comp.cpp:135-159 (Saemundsson; atmos_refrac of hz_shadow.hip), float/double promotions as there.  `fac` = the cell's
// pressure / temperature factor (k_refrac_factor)
__device__ __forceinline__ float horisun_atmos_refrac(float elev_ang_true, double fac) {
    elev_ang_true = __builtin_fmaxf(-1.0f, __builtin_fminf(elev_ang_true, 90.0f));
    float refrac_cor = (float)(1.02 / (double)hz_crm_tanf(horisun_deg2rad_f(
        (float)((double)elev_ang_true + 10.3 / ((double)elev_ang_true + 5.11)))));
    refrac_cor = (float)((double)refrac_cor + 0.0019279);
    refrac_cor = (float)((double)refrac_cor * fac);
    return (float)((double)refrac_cor * (1.0 / 60.0));
}

// Bends the unit sun direction (sun_x, sun_y, sun_z) of an unmasked cell towards its normal and forms dot_prod_ns again from
// the bent direction; the caller forms dot_prod_ts from it.  A cell whose tilted surface faces away from the unrefracted sun
// by more than the refraction can turn it keeps its direction (shadow_setup's exit `dot0 < -bound`, shown there to move no
// result): its dot_prod_ts is then negative, the cell is self-shaded either way, and night positions and back slopes skip
// the libm calls.  A sun at the cell's zenith gives k = 0 / 0: the direction and both dot products come out NaN and the cell is
// self-shaded by `!(dot_ts > 0)`, as in Terrain.
__device__ __forceinline__ void horisun_refract(double fac, float tilt_x, float tilt_y, float tilt_z, float norm_x, float norm_y,
                                                float norm_z, float &sun_x, float &sun_y, float &sun_z, float &dot_prod_ns) {
    {
        const float dot0 = (tilt_x * sun_x + tilt_y * sun_y) + tilt_z * sun_z;
        const float tl = __builtin_fmaxf((tilt_x * tilt_x + tilt_y * tilt_y) + tilt_z * tilt_z, 1.0f);     // >= |tilt|
        const float bound = (0.0114f * __builtin_fabsf((float)fac)) * tl * 1.01f + 1.0e-5f;
        if (dot0 < -bound) return;
    }
    const float elev_ang_true = (float)(90.0 - (double)horisun_rad2deg_f(hz_crm_acosf(dot_prod_ns)));
    const float refrac_cor = horisun_atmos_refrac(elev_ang_true, fac);
    float k_x = sun_y * norm_z - sun_z * norm_y;
    float k_y = sun_z * norm_x - sun_x * norm_z;
    float k_z = sun_x * norm_y - sun_y * norm_x;
    horisun_refrac_unit(k_x, k_y, k_z);
    const float theta = horisun_deg2rad_f(refrac_cor);           // vec_rot, :109-132
    const float ct = hz_crm_cosf(theta), st = hz_crm_sinf(theta);
    const float part = (float)((double)((k_x * sun_x + k_y * sun_y) + k_z * sun_z) * (1.0 - (double)ct));
    const float rx = (sun_x * ct + (k_y * sun_z - k_z * sun_y) * st) + k_x * part;
    const float ry = (sun_y * ct + (k_z * sun_x - k_x * sun_z) * st) + k_y * part;
    const float rz = (sun_z * ct + (k_x * sun_y - k_y * sun_x) * st) + k_z * part;
    sun_x = rx; sun_y = ry; sun_z = rz;
    dot_prod_ns = (norm_x * sun_x + norm_y * sun_y) + norm_z * sun_z;
}

}  // namespace hz

#endif  // HZ_HORISUN_REFRAC_H
