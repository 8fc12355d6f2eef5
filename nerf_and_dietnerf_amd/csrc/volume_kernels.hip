// volume_kernels.hip -- the radiance volume: an (n, n, n, 4) float32 lattice of (r, g, b, sigma) over a box, indexed
// [iz, iy, ix, channel], colour after the sigmoid and density after the ReLU (include/nerf_mi355.h: nerf_radiance_lattice has
// the format, nerf_volume_sample the trilinear rule, nerf_volume_march the march).  Here: the two kernels of the bake that
// mesh_kernels.hip does not have (per-vertex camera directions, raw -> stored texel), the trilinear sampler and the march.
// The network itself runs in nerf_api.hip.
//
// Everything is float32 with every operation rounded on its own (the __f*_rn idiom of aux_kernels.hip), so the numpy
// restatement of tests/volume_ref.py matches the sampler bit for bit and the march up to expf.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "nerf_ctx.h"
#include "ray_box_device.h"

namespace nerf {
namespace {

constexpr int kBs = 256;
unsigned blocks_for(long long items, int bs = kBs) { return (unsigned)((items + bs - 1) / bs); }

__device__ __forceinline__ bool finite_f(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// ---- the bake ----
// The direction the ray generator gives the pixel whose ray passes through point p of camera c (row-major 4x4, looking down
// -z): raygen's direction has camera-space z = -1, so it is (p - t) over the depth of p along the central ray.  A point
// behind the camera (or at it, or a non-finite depth) gets the central ray's direction.
struct CameraArgs { float c[16]; };

__global__ void camera_view_kernel(const CameraArgs cam, const float* __restrict__ xyz, long long count, float* __restrict__ view) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const float* c = cam.c;
    const float qx = __fsub_rn(xyz[3 * t + 0], c[3]), qy = __fsub_rn(xyz[3 * t + 1], c[7]), qz = __fsub_rn(xyz[3 * t + 2], c[11]);
    const float s = -__fadd_rn(__fadd_rn(__fmul_rn(c[2], qx), __fmul_rn(c[6], qy)), __fmul_rn(c[10], qz));
    const bool front = s > 0.0f && finite_f(s);
    view[3 * t + 0] = front ? __fdiv_rn(qx, s) : -c[2];
    view[3 * t + 1] = front ? __fdiv_rn(qy, s) : -c[6];
    view[3 * t + 2] = front ? __fdiv_rn(qz, s) : -c[10];
}

// raw (count, 4) -> the stored texel: the sigmoid of columns 0..2 as raw_rgb_kernel writes it, the ReLU of column 3 as
// composite_terms takes it
__global__ void raw_rgba_kernel(const float* __restrict__ raw, long long count, float* __restrict__ texels) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const float4 o = reinterpret_cast<const float4*>(raw)[t];
    reinterpret_cast<float4*>(texels)[t] = make_float4(1.0f / (1.0f + expf(-o.x)), 1.0f / (1.0f + expf(-o.y)),
                                                       1.0f / (1.0f + expf(-o.z)), fmaxf(o.w, 0.f));
}

// ---- trilinear sampling ----
struct VolumeArgs {
    const float4* texels;
    float lo[3], step[3];
    int n;
};

VolumeArgs volume_args(const float* volume, int n, const float* lo3, const float* hi3) {
    VolumeArgs g;
    g.texels = reinterpret_cast<const float4*>(volume);
    for (int a = 0; a < 3; ++a) {
        g.lo[a] = lo3[a];
        g.step[a] = (hi3[a] - lo3[a]) / (float)(n - 1);      // mesh_kernels.hip::make_lattice's step
    }
    g.n = n;
    return g;
}

// One axis: the cell of coordinate p and the weight of the cell's upper vertex.  The cell is in [0, n - 2] for every input: a
// NaN compares false twice and lands in cell 0 (its weight stays NaN), +-Inf land in the last / first cell with weight 1 / 0.
__device__ __forceinline__ int volume_cell(float p, float lo, float step, int n, float* f) {
    const float g = __fdiv_rn(__fsub_rn(p, lo), step);
    const int i = g >= 0.0f ? (g < (float)(n - 1) ? (int)floorf(g) : n - 2) : 0;
    const float w = __fsub_rn(g, (float)i);
    *f = w < 0.0f ? 0.0f : (w > 1.0f ? 1.0f : w);
    return i;
}

// the eight texels of one cell, index = dx + 2 dy + 4 dz, and the three weights
struct CellFetch {
    float4 v[8];
    float f[3];
};

__device__ __forceinline__ void volume_fetch(const VolumeArgs& g, float px, float py, float pz, CellFetch* c) {
    const int n = g.n;
    const int ix = volume_cell(px, g.lo[0], g.step[0], n, &c->f[0]);
    const int iy = volume_cell(py, g.lo[1], g.step[1], n, &c->f[1]);
    const int iz = volume_cell(pz, g.lo[2], g.step[2], n, &c->f[2]);
    const float4* row = g.texels + ((size_t)iz * n + iy) * n + ix;     // ix + 1, iy + 1, iz + 1 <= n - 1
    const size_t sy = (size_t)n, sz = (size_t)n * n;
    c->v[0] = row[0];       c->v[1] = row[1];
    c->v[2] = row[sy];      c->v[3] = row[sy + 1];
    c->v[4] = row[sz];      c->v[5] = row[sz + 1];
    c->v[6] = row[sz + sy]; c->v[7] = row[sz + sy + 1];
}

__device__ __forceinline__ float lerp_rn(float a, float b, float f) { return __fadd_rn(a, __fmul_rn(f, __fsub_rn(b, a))); }

// along x, then y, then z
__device__ __forceinline__ float trilinear(float v0, float v1, float v2, float v3, float v4, float v5, float v6, float v7,
                                           const float f[3]) {
    const float v00 = lerp_rn(v0, v1, f[0]), v10 = lerp_rn(v2, v3, f[0]);
    const float v01 = lerp_rn(v4, v5, f[0]), v11 = lerp_rn(v6, v7, f[0]);
    return lerp_rn(lerp_rn(v00, v10, f[1]), lerp_rn(v01, v11, f[1]), f[2]);
}

__device__ __forceinline__ float4 volume_value(const CellFetch& c) {
    const float4* v = c.v;
    return make_float4(trilinear(v[0].x, v[1].x, v[2].x, v[3].x, v[4].x, v[5].x, v[6].x, v[7].x, c.f),
                       trilinear(v[0].y, v[1].y, v[2].y, v[3].y, v[4].y, v[5].y, v[6].y, v[7].y, c.f),
                       trilinear(v[0].z, v[1].z, v[2].z, v[3].z, v[4].z, v[5].z, v[6].z, v[7].z, c.f),
                       trilinear(v[0].w, v[1].w, v[2].w, v[3].w, v[4].w, v[5].w, v[6].w, v[7].w, c.f));
}

// one thread per point
__global__ void volume_sample_kernel(const VolumeArgs g, const float* __restrict__ points, long long M, float* __restrict__ out) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= M) return;
    CellFetch c;
    volume_fetch(g, points[3 * t + 0], points[3 * t + 1], points[3 * t + 2], &c);
    reinterpret_cast<float4*>(out)[t] = volume_value(c);
}

// ---- the march ----
// One thread per ray, 64 consecutive rays per wavefront, one wavefront per workgroup: a 256 x 256 frame is 1024 wavefronts,
// one per SIMD of the chip, so what hides the gathers' latency is the work one ray keeps in flight, not other wavefronts.  The
// sample positions do not depend on the transmittance: the ray fetches the cells of kAhead steps (8 x kAhead 16-byte gathers)
// and only then composites them, in order.  A ray under t_min stops fetching at the next group of steps; the steps of its
// last group past the stop, and a last group's steps past n_steps, are fetched (their cells are in the volume like any
// other) and not composited.  kAhead = 4 (161 VGPRs) against 2 and 8 (72, 300): 0.317 ms against 0.357 and 0.314 for the 256 x 256
// frame through n = 256 at 512 steps, 2.80 ms against 2.60 and 4.26 for 1024 x 1024 (profiles/volume_ahead_ab.json).
constexpr int kAhead = 4;

__global__ __launch_bounds__(64) void volume_march_kernel(const VolumeArgs g, const BoxArgs bx, const float* __restrict__ orig,
                                                          const float* __restrict__ dirs, long long N, int n_steps, float t_min,
                                                          float* __restrict__ rgb, float* __restrict__ depth,
                                                          float* __restrict__ opacity) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    const float4 o = reinterpret_cast<const float4*>(orig)[r], d = reinterpret_cast<const float4*>(dirs)[r];
    float a, b;
    bool hit = ray_box_hit(bx, o, d, &a, &b);
    // a ray with a non-finite component is a miss (ray_box_hit does not guard them: a NaN ray would "hit" on [near, far])
    hit = hit && finite_f(o.x) && finite_f(o.y) && finite_f(o.z) && finite_f(d.x) && finite_f(d.y) && finite_f(d.z);
    float cr = 0.0f, cg = 0.0f, cb = 0.0f, cd = 0.0f, T = 1.0f;
    if (hit) {
        const float delta = __fdiv_rn(__fsub_rn(b, a), (float)n_steps);
        bool alive = true;
        for (int k0 = 0; k0 < n_steps && alive; k0 += kAhead) {
            CellFetch c[kAhead];
            float z[kAhead];
#pragma unroll
            for (int u = 0; u < kAhead; ++u) {
                z[u] = __fadd_rn(a, __fmul_rn(__fadd_rn((float)(k0 + u), 0.5f), delta));
                volume_fetch(g, __fadd_rn(o.x, __fmul_rn(d.x, z[u])), __fadd_rn(o.y, __fmul_rn(d.y, z[u])),
                             __fadd_rn(o.z, __fmul_rn(d.z, z[u])), &c[u]);
            }
#pragma unroll
            for (int u = 0; u < kAhead; ++u) {
                const float4 v = volume_value(c[u]);
                const float e = expf(-__fmul_rn(v.w, delta));
                const float alpha = __fsub_rn(1.0f, e);
                const float w = __fmul_rn(alpha, T);
                const bool on = alive && k0 + u < n_steps;          // predicated, not branched: the body is a few selects
                cr = on ? __fadd_rn(cr, __fmul_rn(w, v.x)) : cr;
                cg = on ? __fadd_rn(cg, __fmul_rn(w, v.y)) : cg;
                cb = on ? __fadd_rn(cb, __fmul_rn(w, v.z)) : cb;
                cd = on ? __fadd_rn(cd, __fmul_rn(w, z[u])) : cd;
                T = on ? __fmul_rn(T, __fsub_rn(1.0f, alpha)) : T;
                alive = alive && !(on && T < t_min);
            }
        }
    }
    if (rgb) { rgb[3 * r + 0] = cr; rgb[3 * r + 1] = cg; rgb[3 * r + 2] = cb; }
    if (depth) depth[r] = cd;
    if (opacity) opacity[r] = __fsub_rn(1.0f, T);
}

}  // namespace

void launch_camera_view(const float c2w[16], const float* xyz, long long count, float* view, hipStream_t stream) {
    if (count <= 0) return;
    CameraArgs cam;
    for (int i = 0; i < 16; ++i) cam.c[i] = c2w[i];
    hipLaunchKernelGGL(camera_view_kernel, dim3(blocks_for(count)), dim3(kBs), 0, stream, cam, xyz, count, view);
}

void launch_raw_rgba(const float* raw, long long count, float* texels, hipStream_t stream) {
    if (count <= 0) return;
    hipLaunchKernelGGL(raw_rgba_kernel, dim3(blocks_for(count)), dim3(kBs), 0, stream, raw, count, texels);
}

void launch_volume_sample(const float* volume, int n, const float* lo3, const float* hi3, const float* points, long long M,
                          float* out, hipStream_t stream) {
    if (M <= 0) return;
    hipLaunchKernelGGL(volume_sample_kernel, dim3(blocks_for(M)), dim3(kBs), 0, stream, volume_args(volume, n, lo3, hi3), points,
                       M, out);
}

void launch_volume_march(const float* volume, int n, const float* lo3, const float* hi3, float near_b, float far_b,
                         const float* orig, const float* dirs, long long N, int n_steps, float t_min, float* rgb, float* depth,
                         float* opacity, hipStream_t stream) {
    if (N <= 0) return;
    SceneBox box;
    for (int a = 0; a < 3; ++a) { box.lo[a] = lo3[a]; box.hi[a] = hi3[a]; }
    hipLaunchKernelGGL(volume_march_kernel, dim3(blocks_for(N, 64)), dim3(64), 0, stream, volume_args(volume, n, lo3, hi3),
                       box_args(box, near_b, far_b), orig, dirs, N, n_steps, t_min, rgb, depth, opacity);
}

}  // namespace nerf
