// ray_box_device.h -- the scene-box rule as device functions, for every translation unit that clips a ray to a box
// (aux_kernels.hip: the depth kernels, nerf_ray_box_bounds, the occupancy walk; volume_kernels.hip: the volume march).  Device
// functions do not cross translation units in this build, so the one statement of the rule lives here.
//
// Scene box: the interval of a ray (o, d) inside an axis-aligned box lo < hi, clipped to
// [near, far].  Depths are the parameter t of o + t d; d is not normalised.  float32, every operation rounded on its own:
//   1. per axis with d_a != 0: t0 = (lo_a - o_a) / d_a, t1 = (hi_a - o_a) / d_a, axis interval [min, max]
//   2. per axis with d_a == 0 (either zero): no constraint if lo_a <= o_a <= hi_a, otherwise the ray misses -- a branch,
//      not the NaN of 0 / 0, which would turn "on the face" into a miss
//   3. tn = largest lower end, tf = smallest upper end; a = max(tn, near), b = min(tf, far)
//   4. hit: no axis missed and b > a.  NARROWED: hit and (a > near or b < far)
// min / max are written as comparisons: nothing hangs on how fminf / fmaxf treat NaN or the sign of zero (non-finite rays
// are not guarded, as in rays_to_ndc).  -> narrowed; a, b are meant to be used only then.
#pragma once
#include <hip/hip_runtime.h>

#include "nerf_kernels.h"

namespace nerf {

struct BoxArgs {
    float lo[3], hi[3];
    float near_b, far_b;
};

inline BoxArgs box_args(const SceneBox& box, float near_b, float far_b) {
    BoxArgs bx;
    for (int i = 0; i < 3; ++i) { bx.lo[i] = box.lo[i]; bx.hi[i] = box.hi[i]; }
    bx.near_b = near_b; bx.far_b = far_b;
    return bx;
}

// steps 1-3 and the first half of 4: -> hit; (a, b) = the ray clipped to the box and to near / far
__device__ __forceinline__ bool ray_box_hit(const BoxArgs& bx, const float4 o, const float4 d, float* a, float* b) {
    const float oo[3] = {o.x, o.y, o.z}, dd[3] = {d.x, d.y, d.z};
    float tn = -__builtin_huge_valf(), tf = __builtin_huge_valf();
    bool miss = false;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        if (dd[ax] == 0.0f) {
            if (!(bx.lo[ax] <= oo[ax] && oo[ax] <= bx.hi[ax])) miss = true;
            continue;
        }
        const float t0 = __fdiv_rn(__fsub_rn(bx.lo[ax], oo[ax]), dd[ax]);
        const float t1 = __fdiv_rn(__fsub_rn(bx.hi[ax], oo[ax]), dd[ax]);
        const bool first = t0 < t1;
        const float low = first ? t0 : t1, high = first ? t1 : t0;
        if (low > tn) tn = low;
        if (high < tf) tf = high;
    }
    *a = tn > bx.near_b ? tn : bx.near_b;
    *b = tf < bx.far_b ? tf : bx.far_b;
    return !miss && *b > *a;
}

__device__ __forceinline__ bool ray_box_interval(const BoxArgs& bx, const float4 o, const float4 d, float* a, float* b) {
    const bool hit = ray_box_hit(bx, o, d, a, b);
    return hit && (*a > bx.near_b || *b < bx.far_b);
}

}  // namespace nerf
