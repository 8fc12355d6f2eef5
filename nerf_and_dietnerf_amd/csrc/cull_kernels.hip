// cull_kernels.hip -- sample culling under an occupancy grid (include/nerf_mi355.h: nerf_ctx_set_sample_culling has the
// rule): the samples of a render pass that lie in empty cells of the grid never reach the network.  sample_kept decides per
// sample, sample_keep_kernel packs the verdicts into a bit mask, mesh_kernels.hip's scan turns the mask into a slot per kept
// sample and the row count M, sample_gather_kernel writes the kept samples' points as the M rows of a point-mode (mode 1)
// network pass, and raw_expand_kernel spreads the M raw rows back over all N * S samples with zeros for the culled ones.
//
// The trainer under nerf_ctx_set_train_sample_culling (train_api.hip) uses the same kernels for its forward half; its backward
// half adds graw_gather_kernel (the kept rows of dL/d(raw), padded to whole 128-row tiles with zero rows) and hands the mask
// and the slots to train_kernels.hip's pe_bwd_kernel, which then reads the encoding gradient of sample t at its compact row.
//
// Canonical like the mesh: no atomics, the rows are in ascending sample index (nerf_device.h: sample_slot).  The fused MLP
// kernels are not touched: they take M by value, so the host reads it (nerf_api.hip: compact_samples, the one routine both
// paths call).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "field_device.h"
#include "nerf_device.h"
#include "nerf_kernels.h"

namespace nerf {
namespace {

struct CullArgs {
    float lo[3], hi[3], cell[3];   // cell_a = (hi_a - lo_a) / R, float32
    const uint32_t* bits;          // R^3 / 32 words, cell (ix, iy, iz) = bit ix + R (iy + R iz)
    int R;
};

CullArgs cull_args(const SceneBox& box, const uint32_t* bits, int R) {
    CullArgs g;
    for (int a = 0; a < 3; ++a) {
        g.lo[a] = box.lo[a]; g.hi[a] = box.hi[a];
        g.cell[a] = (box.hi[a] - box.lo[a]) / (float)R;
    }
    g.bits = bits; g.R = R;
    return g;
}

// The verdict of one sample: float32, every operation rounded on its own, comparisons instead of fminf / fmaxf.
//   1. p_a = o_a + d_a z, multiply then add: the point the MLP kernels form in mode 0, bit for bit
//   2. inside = lo_a <= p_a <= hi_a on all three axes (a NaN compares false: not inside)
//   3. i_a = clamp(floor((p_a - lo_a) / cell_a), 0, R - 1), grid_cell_index (nerf_device.h), which ray_grid_interval calls too:
//      the hi face belongs to cell R - 1, an interior cell face to the upper cell
//   4. culled iff inside and the cell's bit is 0.  A sample outside the box is kept: the grid knows nothing there.
// -> kept.  p: the point of step 1.
__device__ __forceinline__ bool sample_kept(const CullArgs& g, const float4 o, const float4 d, float z, float p[3]) {
    const float oo[3] = {o.x, o.y, o.z}, dd[3] = {d.x, d.y, d.z};
    const int R = g.R;
    bool inside = true;
    int idx[3];
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        p[ax] = __fadd_rn(oo[ax], __fmul_rn(dd[ax], z));
        if (!(g.lo[ax] <= p[ax] && p[ax] <= g.hi[ax])) inside = false;
        idx[ax] = grid_cell_index(p[ax], g.lo[ax], g.cell[ax], R);    // NaN -> 0: the index is in [0, R) whatever p is
    }
    if (!inside) return true;
    const int bit = idx[0] + R * (idx[1] + R * idx[2]);           // < R^3 <= 2^24
    return ((g.bits[bit >> 5] >> (bit & 31)) & 1u) != 0;
}

// One thread per sample; a wave's 64 verdicts are one ballot, stored by its first lane.  Tail lanes vote 0, so the mask's
// last word is whole.  mask: ceil(total / 64) words (nullable); verdict: (total,) int32 1 kept / 0 culled (nullable).
__global__ __launch_bounds__(kBs) void sample_keep_kernel(const CullArgs g, const float* __restrict__ orig,
                                                          const float* __restrict__ dirs, const float* __restrict__ z,
                                                          long long total, int S, unsigned long long* __restrict__ mask,
                                                          int* __restrict__ verdict) {
    const long long t = (long long)blockIdx.x * kBs + threadIdx.x;
    bool keep = false;
    if (t < total) {
        const long long r = t / S;
        float p[3];
        keep = sample_kept(g, reinterpret_cast<const float4*>(orig)[r], reinterpret_cast<const float4*>(dirs)[r], z[t], p);
        if (verdict) verdict[t] = keep ? 1 : 0;
    }
    const unsigned long long m = __ballot(keep);
    if (mask && (threadIdx.x & 63) == 0 && t < total) mask[t >> 6] = m;
}

// One thread per sample: a kept sample writes its point (step 1's operations) and its ray's direction to its slot.
__global__ __launch_bounds__(kBs) void sample_gather_kernel(const float* __restrict__ orig, const float* __restrict__ dirs,
                                                            const float* __restrict__ z, long long total, int S,
                                                            const uint8_t* __restrict__ mask, const uint32_t* __restrict__ first,
                                                            float* __restrict__ xyz, float* __restrict__ view) {
    const long long t = (long long)blockIdx.x * kBs + threadIdx.x;
    if (t >= total) return;
    size_t slot;
    if (!sample_slot(mask, first, t, &slot)) return;
    const long long r = t / S;
    const float4 o = reinterpret_cast<const float4*>(orig)[r], d = reinterpret_cast<const float4*>(dirs)[r];
    const float zz = z[t];
    xyz[3 * slot + 0] = __fadd_rn(o.x, __fmul_rn(d.x, zz));
    xyz[3 * slot + 1] = __fadd_rn(o.y, __fmul_rn(d.y, zz));
    xyz[3 * slot + 2] = __fadd_rn(o.z, __fmul_rn(d.z, zz));
    if (view) { view[3 * slot + 0] = d.x; view[3 * slot + 1] = d.y; view[3 * slot + 2] = d.z; }
}

// One thread per sample: the full raw buffer from the compact rows, zeros for a culled sample.  SIGMA: (total,) sigma from
// (M,) sigma (the sigma-only coarse pass); otherwise (total, 4) from (M, 4).
template <bool SIGMA>
__global__ __launch_bounds__(kBs) void raw_expand_kernel(const float* __restrict__ compact, long long total,
                                                         const uint8_t* __restrict__ mask, const uint32_t* __restrict__ first,
                                                         float* __restrict__ raw) {
    const long long t = (long long)blockIdx.x * kBs + threadIdx.x;
    if (t >= total) return;
    size_t slot;
    const bool kept = sample_slot(mask, first, t, &slot);
    if constexpr (SIGMA) raw[t] = kept ? compact[slot] : 0.f;
    else reinterpret_cast<float4*>(raw)[t] = kept ? reinterpret_cast<const float4*>(compact)[slot] : make_float4(0.f, 0.f, 0.f, 0.f);
}

// The kept rows of Graw (total, 4) as the compact (Mp, 4) buffer the backward passes read; its padding rows M .. Mp are zero.
// One thread per sample, then one per padding row.
__global__ __launch_bounds__(kBs) void graw_gather_kernel(const float* __restrict__ graw, long long total, long long M,
                                                          long long Mp, const uint8_t* __restrict__ mask,
                                                          const uint32_t* __restrict__ first, float* __restrict__ compact) {
    const long long t = (long long)blockIdx.x * kBs + threadIdx.x;
    if (t < total) {
        size_t slot;
        if (sample_slot(mask, first, t, &slot)) reinterpret_cast<float4*>(compact)[slot] = reinterpret_cast<const float4*>(graw)[t];
    } else if (t - total < Mp - M) {
        reinterpret_cast<float4*>(compact)[M + (t - total)] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

}  // namespace

void launch_sample_keep(const SceneBox& box, const uint32_t* bits, int R, const float* orig, const float* dirs, const float* z,
                        long long N, int S, uint64_t* mask, int* verdict, hipStream_t stream) {
    const long long total = N * S;
    if (total <= 0) return;
    hipLaunchKernelGGL(sample_keep_kernel, dim3(blocks_for(total)), dim3(kBs), 0, stream, cull_args(box, bits, R), orig, dirs, z,
                       total, S, (unsigned long long*)mask, verdict);
}

void launch_sample_gather(const float* orig, const float* dirs, const float* z, long long N, int S, const uint8_t* mask,
                          const uint32_t* first, float* xyz, float* view, hipStream_t stream) {
    const long long total = N * S;
    if (total <= 0) return;
    hipLaunchKernelGGL(sample_gather_kernel, dim3(blocks_for(total)), dim3(kBs), 0, stream, orig, dirs, z, total, S, mask, first,
                       xyz, view);
}

void launch_raw_expand(const float* compact, long long total, bool sigma_only, const uint8_t* mask, const uint32_t* first,
                       float* raw, hipStream_t stream) {
    if (total <= 0) return;
    if (sigma_only)
        hipLaunchKernelGGL(raw_expand_kernel<true>, dim3(blocks_for(total)), dim3(kBs), 0, stream, compact, total, mask, first, raw);
    else
        hipLaunchKernelGGL(raw_expand_kernel<false>, dim3(blocks_for(total)), dim3(kBs), 0, stream, compact, total, mask, first, raw);
}

void launch_graw_gather(const float* graw, long long total, long long M, long long Mp, const uint8_t* mask, const uint32_t* first,
                        float* compact, hipStream_t stream) {
    const long long items = total + (Mp - M);
    if (items <= 0) return;
    hipLaunchKernelGGL(graw_gather_kernel, dim3(blocks_for(items)), dim3(kBs), 0, stream, graw, total, M, Mp, mask, first, compact);
}

}  // namespace nerf
