// field_kernels.hip -- the small kernels on either side of the network in a field query (field_api.hip has the loop): the
// fills write a chunk's points and view directions, the drains rework its raw rows.  float32 with every operation rounded
// on its own (the __f*_rn idiom of aux_kernels.hip), so the tests' numpy restatements match the points bit for bit.
#include "field_device.h"
#include "nerf_kernels.h"
#include "ray_box_device.h"
#include "sampling_device.h"

namespace nerf {

// ---- occupancy bake: cell sample points -> the network's sigma -> bits -> dilation ----
// Cells are numbered as their bits are.  A chunk is a run of whole 64-cell groups [cell_begin, cell_begin + n_cells), so a
// wavefront's ballot is two whole words.  Point j of a cell: j == 0 the centre lo + cell (i + 0.5), j > 0 lo + cell (i + u)
// with u = Philox(seed, cell number, 3 j + axis), stream 2 (the depth draws use 0 and 1).  The view direction is the unit
// vector (0, 0, 1): sigma does not depend on it.
__global__ void grid_points_kernel(const BoxArgs bx, int R, long long cell_begin, long long n_points, int spc, uint64_t seed,
                                   float* __restrict__ xyz, float* __restrict__ view) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_points) return;
    const long long cell = cell_begin + p / spc;
    const int j = (int)(p % spc);
    const int i[3] = {(int)(cell % R), (int)((cell / R) % R), (int)(cell / ((long long)R * R))};
    float x[3];
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        const float w = __fdiv_rn(__fsub_rn(bx.hi[ax], bx.lo[ax]), (float)R);
        const float f = j == 0 ? 0.5f : philox_uniform(seed, (uint64_t)cell, 3 * j + ax, 2u);
        x[ax] = __fadd_rn(bx.lo[ax], __fmul_rn(w, __fadd_rn((float)i[ax], f)));
    }
    xyz[3 * p + 0] = x[0]; xyz[3 * p + 1] = x[1]; xyz[3 * p + 2] = x[2];
    if (view) { view[3 * p + 0] = 0.f; view[3 * p + 1] = 0.f; view[3 * p + 2] = 1.f; }
}

// raw (n_cells * spc, 4): column 3 is sigma.  One thread per cell; lanes 0 and 32 of a wavefront store its two words.
__global__ void grid_threshold_kernel(const float* __restrict__ raw, long long cell_begin, long long n_cells, int spc,
                                      float threshold, uint32_t* __restrict__ bits) {
    const long long cl = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    bool occ = false;
    if (cl < n_cells) {
        float m = raw[4 * (cl * spc) + 3];
        for (int j = 1; j < spc; ++j) {
            const float v = raw[4 * (cl * spc + j) + 3];
            if (v > m) m = v;
        }
        occ = m > threshold;      // NaN: empty
    }
    const unsigned long long vote = __ballot(occ);
    const int lane = threadIdx.x & 63;
    if (cl < n_cells && (lane & 31) == 0) bits[(cell_begin + cl) >> 5] = (uint32_t)(vote >> lane);
}

// dst = src grown by one cell in the 26-neighbourhood.  One thread per cell, R^3 a multiple of 64.
__global__ void grid_dilate_kernel(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, int R) {
    const long long cells = (long long)R * R * R;
    const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    bool occ = false;
    if (c < cells) {
        const int ix = (int)(c % R), iy = (int)((c / R) % R), iz = (int)(c / ((long long)R * R));
        for (int dz = -1; dz <= 1; ++dz)
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    const int x = ix + dx, y = iy + dy, zc = iz + dz;
                    if (x < 0 || x >= R || y < 0 || y >= R || zc < 0 || zc >= R) continue;
                    const int bit = x + R * (y + R * zc);
                    occ = occ || ((src[bit >> 5] >> (bit & 31)) & 1u);
                }
    }
    const unsigned long long vote = __ballot(occ);
    const int lane = threadIdx.x & 63;
    if (c < cells && (lane & 31) == 0) dst[c >> 5] = (uint32_t)(vote >> lane);
}

namespace {

// ---- the lattice the network is evaluated on (field_device.h) ----
__global__ void lattice_points_kernel(const Lattice l, long long begin, long long count, float vx, float vy, float vz,
                                      float* __restrict__ xyz, float* __restrict__ view) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const long long p = begin + t;
    const int n = l.n;
    const int i[3] = {(int)(p % n), (int)((p / n) % n), (int)(p / ((long long)n * n))};
    xyz[3 * t + 0] = lattice_coord(l, 0, i[0]);
    xyz[3 * t + 1] = lattice_coord(l, 1, i[1]);
    xyz[3 * t + 2] = lattice_coord(l, 2, i[2]);
    if (view) { view[3 * t + 0] = vx; view[3 * t + 1] = vy; view[3 * t + 2] = vz; }
}

// raw (count, 4) -> its column 3
__global__ void raw_sigma_kernel(const float* __restrict__ raw, long long count, float* __restrict__ sigma) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < count) sigma[t] = raw[4 * t + 3];
}

// vertex colours: the direction a ray that sees the surface travels in, against the normal; a zero normal looks down +z
__global__ void mesh_view_kernel(const float* __restrict__ normals, long long count, float* __restrict__ view) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const float x = normals[3 * t], y = normals[3 * t + 1], z = normals[3 * t + 2];
    const bool zero = x == 0.f && y == 0.f && z == 0.f;
    view[3 * t + 0] = zero ? 0.f : -x;
    view[3 * t + 1] = zero ? 0.f : -y;
    view[3 * t + 2] = zero ? 1.f : -z;
}

// raw (count, 4) -> the colour of columns 0..2, as composite_kernel writes rgb_samples
__global__ void raw_rgb_kernel(const float* __restrict__ raw, long long count, float* __restrict__ rgb) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const float4 o = reinterpret_cast<const float4*>(raw)[t];
    rgb[3 * t + 0] = raw_sigmoid(o.x);
    rgb[3 * t + 1] = raw_sigmoid(o.y);
    rgb[3 * t + 2] = raw_sigmoid(o.z);
}

// radiance lattice.  The direction the ray generator gives the pixel whose ray passes through point p of camera c (row-major
// 4x4, looking down -z): raygen's direction has camera-space z = -1, so it is (p - t) over the depth of p along the central
// ray.  A point behind the camera (or at it, or a non-finite depth) gets the central ray's direction.
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

// raw (count, 4) -> the stored texel: the colour of columns 0..2 and the ReLU of column 3, both as composite_terms takes them
__global__ void raw_rgba_kernel(const float* __restrict__ raw, long long count, float* __restrict__ texels) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const float4 o = reinterpret_cast<const float4*>(raw)[t];
    reinterpret_cast<float4*>(texels)[t] = make_float4(raw_sigmoid(o.x), raw_sigmoid(o.y), raw_sigmoid(o.z), fmaxf(o.w, 0.f));
}

// ---- SH radiance lattice (nerf_sh_radiance_lattice has the rule) ----
// the fill: point p of a chunk is vertex begin + p / D seen along direction p % D of the table (D, 3), as given
__global__ void sh_lattice_points_kernel(const Lattice l, long long begin, long long count, int D, const float* __restrict__ table,
                                         float* __restrict__ xyz, float* __restrict__ view) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const long long p = begin + t / D;
    const int j = (int)(t % D), n = l.n;
    const int i[3] = {(int)(p % n), (int)((p / n) % n), (int)(p / ((long long)n * n))};
    xyz[3 * t + 0] = lattice_coord(l, 0, i[0]);
    xyz[3 * t + 1] = lattice_coord(l, 1, i[1]);
    xyz[3 * t + 2] = lattice_coord(l, 2, i[2]);
    if (view) { view[3 * t + 0] = table[3 * j]; view[3 * t + 1] = table[3 * j + 1]; view[3 * t + 2] = table[3 * j + 2]; }
}

// the drain: raw (count * D, 4) -> texels (count, C(L)).  One thread per vertex; the K x 3 sums stay in registers, each
// fed in the order of j; proj (K, D) is read at wave-uniform addresses.
template <int L>
__global__ void sh_project_kernel(const float* __restrict__ raw, long long count, int D, const float* __restrict__ proj,
                                  float* __restrict__ texels) {
    constexpr int K = sh_basis_count(L), C = sh_texel_floats(L);
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const float4* rows = reinterpret_cast<const float4*>(raw) + t * D;
    float coef[3 * K];
    float sigma = 0.f;
    for (int j = 0; j < D; ++j) {
        const float4 o = rows[j];
        const float col[3] = {raw_sigmoid(o.x), raw_sigmoid(o.y), raw_sigmoid(o.z)};
        if (j == 0) sigma = fmaxf(o.w, 0.f);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float w = proj[(size_t)k * D + j];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const float term = __fmul_rn(w, col[ch]);
                coef[3 * k + ch] = j == 0 ? term : __fadd_rn(coef[3 * k + ch], term);
            }
        }
    }
    float4* out = reinterpret_cast<float4*>(texels + (size_t)t * C);
#pragma unroll
    for (int q = 0; q < C / 4; ++q) {
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int ch = 4 * q + e;
            v[e] = ch < 3 * K ? coef[ch < 3 * K ? ch : 0] : (ch == 3 * K ? sigma : 0.f);
        }
        out[q] = make_float4(v[0], v[1], v[2], v[3]);
    }
}

}  // namespace

void launch_grid_points(const SceneBox& box, int R, long long cell_begin, long long n_cells, int spc, uint64_t seed,
                        float* xyz, float* view, hipStream_t stream) {
    const long long n_points = n_cells * spc;
    if (n_points <= 0) return;
    hipLaunchKernelGGL(grid_points_kernel, dim3(blocks_for(n_points)), dim3(kBs), 0, stream, box_args(box, 0.f, 0.f), R,
                       cell_begin, n_points, spc, seed, xyz, view);
}

void launch_grid_threshold(const float* raw, long long cell_begin, long long n_cells, int spc, float threshold,
                           uint32_t* bits, hipStream_t stream) {
    if (n_cells <= 0) return;
    hipLaunchKernelGGL(grid_threshold_kernel, dim3(blocks_for(n_cells)), dim3(kBs), 0, stream, raw, cell_begin, n_cells, spc,
                       threshold, bits);
}

void launch_grid_dilate(const uint32_t* src, uint32_t* dst, int R, hipStream_t stream) {
    hipLaunchKernelGGL(grid_dilate_kernel, dim3(blocks_for((long long)R * R * R)), dim3(kBs), 0, stream, src, dst, R);
}

void launch_lattice_points(const SceneBox& box, int n, long long begin, long long count, const float view_dir[3], float* xyz,
                           float* view, hipStream_t stream) {
    if (count <= 0) return;
    hipLaunchKernelGGL(lattice_points_kernel, dim3(blocks_for(count)), dim3(kBs), 0, stream, make_lattice(box.lo, box.hi, n),
                       begin, count, view_dir[0], view_dir[1], view_dir[2], xyz, view);
}

void launch_raw_sigma(const float* raw, long long count, float* sigma, hipStream_t stream) {
    if (count > 0) hipLaunchKernelGGL(raw_sigma_kernel, dim3(blocks_for(count)), dim3(kBs), 0, stream, raw, count, sigma);
}
void launch_mesh_view(const float* normals, long long count, float* view, hipStream_t stream) {
    if (count > 0) hipLaunchKernelGGL(mesh_view_kernel, dim3(blocks_for(count)), dim3(kBs), 0, stream, normals, count, view);
}
void launch_raw_rgb(const float* raw, long long count, float* rgb, hipStream_t stream) {
    if (count > 0) hipLaunchKernelGGL(raw_rgb_kernel, dim3(blocks_for(count)), dim3(kBs), 0, stream, raw, count, rgb);
}

void launch_camera_view(const float c2w[16], const float* xyz, long long count, float* view, hipStream_t stream) {
    if (count <= 0) return;
    CameraArgs cam;
    for (int i = 0; i < 16; ++i) cam.c[i] = c2w[i];
    hipLaunchKernelGGL(camera_view_kernel, dim3(blocks_for(count)), dim3(kBs), 0, stream, cam, xyz, count, view);
}

void launch_raw_rgba(const float* raw, long long count, float* texels, hipStream_t stream) {
    if (count > 0) hipLaunchKernelGGL(raw_rgba_kernel, dim3(blocks_for(count)), dim3(kBs), 0, stream, raw, count, texels);
}

void launch_sh_lattice_points(const SceneBox& box, int n, long long begin, long long count, int D, const float* table, float* xyz,
                              float* view, hipStream_t stream) {
    if (count <= 0) return;
    hipLaunchKernelGGL(sh_lattice_points_kernel, dim3(blocks_for(count * D)), dim3(kBs), 0, stream,
                       make_lattice(box.lo, box.hi, n), begin, count * D, D, table, xyz, view);
}

void launch_sh_project(const float* raw, long long count, int degree, int D, const float* proj, float* texels, hipStream_t stream) {
    if (count <= 0) return;
    const dim3 grid(blocks_for(count)), block(kBs);
    switch (degree) {
        case 0: hipLaunchKernelGGL(sh_project_kernel<0>, grid, block, 0, stream, raw, count, D, proj, texels); break;
        case 1: hipLaunchKernelGGL(sh_project_kernel<1>, grid, block, 0, stream, raw, count, D, proj, texels); break;
        case 2: hipLaunchKernelGGL(sh_project_kernel<2>, grid, block, 0, stream, raw, count, D, proj, texels); break;
        default: hipLaunchKernelGGL(sh_project_kernel<3>, grid, block, 0, stream, raw, count, D, proj, texels); break;
    }
}

}  // namespace nerf
