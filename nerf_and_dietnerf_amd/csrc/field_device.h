// field_device.h -- the lattice over a box, stated once for every translation unit that lays points on it or reads a volume
// stored on it (field_kernels.hip: the network's points; mesh_kernels.hip: the isosurface; volume_kernels.hip: the sampler and
// the march), and the launch geometry of one-thread-per-item kernels.  Device functions do not cross translation units here.
#pragma once
#include <hip/hip_runtime.h>

namespace nerf {

constexpr int kBs = 256;
inline unsigned blocks_for(long long items, int bs = kBs) { return (unsigned)((items + bs - 1) / bs); }

// n points per axis, point i of an axis at lo + step * i: the first on the box's lower face, the last (up to rounding) on its upper
struct Lattice { float lo[3], step[3]; int n; };

inline Lattice make_lattice(const float* lo3, const float* hi3, int n) {
    Lattice l;
    for (int a = 0; a < 3; ++a) { l.lo[a] = lo3[a]; l.step[a] = (hi3[a] - lo3[a]) / (float)(n - 1); }
    l.n = n;
    return l;
}

__device__ __forceinline__ float lattice_coord(const Lattice& l, int axis, int i) {
    return __fadd_rn(l.lo[axis], __fmul_rn(l.step[axis], (float)i));
}

__device__ __forceinline__ bool finite_f(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// The SH volume's texel (include/nerf_mi355.h: nerf_sh_radiance_lattice has the format): K basis functions of degree L,
// 3 K coefficients, sigma, zeros up to a multiple of 4 floats -- 4 / 16 / 28 / 52.
constexpr int kShMaxDegree = 3, kShMaxDirs = 64;
__host__ __device__ constexpr int sh_basis_count(int degree) { return (degree + 1) * (degree + 1); }
__host__ __device__ constexpr int sh_texel_floats(int degree) { return 4 * ((3 * sh_basis_count(degree) + 1 + 3) / 4); }

}  // namespace nerf
