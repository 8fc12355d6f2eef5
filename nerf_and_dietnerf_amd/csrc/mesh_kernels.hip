// mesh_kernels.hip -- a triangle mesh out of the density field: the isosurface of an n^3 volume over a lattice
// (field_device.h) by marching tetrahedra (nerf_isosurface / nerf_isosurface_fetch, include/nerf_mi355.h has the rule), and
// the exclusive scan it numbers its output with.  The network on the lattice and at the vertices: field_api.hip.
//
// The isosurface is canonical: no atomics, no hashing.  Every output slot is known from two exclusive scans -- the crossed
// edges of every lattice point, the triangles of every cube -- so a vertex id is (first id of the edge's base point) + (rank
// of the edge's type among that point's crossed edges), and the numpy restatement of the tests matches it bit for bit.
// Positions and normals are float32 with every operation rounded on its own (the __f*_rn idiom of aux_kernels.hip).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "field_device.h"
#include "nerf_ctx.h"

namespace nerf {
namespace {

// ---- marching tetrahedra ----
// Edge types in key order: 100, 010, 001, 110, 011, 101, 111 as (dx, dy, dz).
__device__ __constant__ const signed char kEdge[7][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {1, 1, 0}, {0, 1, 1}, {1, 0, 1}, {1, 1, 1}};
// type of the edge with offset code dx + 2 dy + 4 dz (1..7)
__device__ __constant__ const signed char kTypeOfCode[8] = {-1, 0, 1, 3, 2, 5, 4, 6};
// the six axis permutations in lexicographic order, and their parity (1: odd)
__device__ __constant__ const signed char kPerm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
constexpr unsigned kPermOdd = 0x26;   // bits 1, 2, 5
// Orientation, decided from the case alone.  A tetrahedron c0, c1 = c0 + e_a, c2 = c1 + e_b, c3 = c2 + e_c has
// det(c1 - c0, c2 - c0, c3 - c0) = det(e_a, e_b, e_c) = the sign of the permutation.  For an EVEN permutation the polygon in
// the rule's order (bit i of the case = corner i inside) runs clockwise seen from the outside -- and is reversed -- in these
// cases: one corner k inside and k odd (cases 2, 8); one corner k outside and k even (cases 11, 14); the inside pairs {0, 2}
// and {1, 3} (cases 5, 10).  An odd permutation mirrors the tetrahedron: every other case of 1..14 is reversed instead.
constexpr unsigned kFlipEven = 0x4d24;

__device__ __forceinline__ bool inside(float s, float iso) { return s > iso; }   // NaN: outside

// bit t of mask[p]: the edge of type t at lattice point p lies in the lattice and its two ends differ in "inside"
__global__ void iso_point_mask_kernel(const float* __restrict__ s, int n, float iso, uint8_t* __restrict__ mask) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long total = (long long)n * n * n;
    if (p >= total) return;
    const int ix = (int)(p % n), iy = (int)((p / n) % n), iz = (int)(p / ((long long)n * n));
    const bool in0 = inside(s[p], iso);
    unsigned m = 0;
#pragma unroll
    for (int t = 0; t < 7; ++t) {
        const int dx = kEdge[t][0], dy = kEdge[t][1], dz = kEdge[t][2];
        if (ix + dx >= n || iy + dy >= n || iz + dz >= n) continue;
        const bool in1 = inside(s[p + dx + (long long)n * (dy + (long long)n * dz)], iso);
        m |= (unsigned)(in0 != in1) << t;
    }
    mask[p] = (uint8_t)m;
}

// the 8 corners of cube (cx, cy, cz) as bits dx + 2 dy + 4 dz
__device__ __forceinline__ unsigned cube_inside_bits(const float* __restrict__ s, int n, float iso, long long base) {
    unsigned bits = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const long long q = base + (k & 1) + (long long)n * (((k >> 1) & 1) + (long long)n * (k >> 2));
        bits |= (unsigned)inside(s[q], iso) << k;
    }
    return bits;
}

// case of tetrahedron `perm` (bit i: corner i inside) and the offset codes of its corners
__device__ __forceinline__ unsigned tet_case(unsigned cube_bits, int perm, int code[4]) {
    code[0] = 0;
    code[1] = 1 << kPerm[perm][0];
    code[2] = code[1] | (1 << kPerm[perm][1]);
    code[3] = 7;
    return ((cube_bits >> code[0]) & 1u) | (((cube_bits >> code[1]) & 1u) << 1) | (((cube_bits >> code[2]) & 1u) << 2) |
           (((cube_bits >> code[3]) & 1u) << 3);
}

__device__ __forceinline__ int tet_triangles(unsigned cs) {
    const int k = __popc(cs);
    return k == 2 ? 2 : (k == 1 || k == 3) ? 1 : 0;
}

__global__ void iso_cube_count_kernel(const float* __restrict__ s, int n, float iso, uint8_t* __restrict__ count) {
    const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int m = n - 1;
    if (c >= (long long)m * m * m) return;
    const int cx = (int)(c % m), cy = (int)((c / m) % m), cz = (int)(c / ((long long)m * m));
    const unsigned bits = cube_inside_bits(s, n, iso, cx + (long long)n * (cy + (long long)n * cz));
    int total = 0;
    if (bits != 0 && bits != 0xff) {
#pragma unroll
        for (int perm = 0; perm < 6; ++perm) {
            int code[4];
            total += tet_triangles(tet_case(bits, perm, code));
        }
    }
    count[c] = (uint8_t)total;
}

// d s / d axis at lattice point p (index i along the axis, element stride `stride`): central, one-sided at the faces
__device__ __forceinline__ float lattice_gradient(const float* __restrict__ s, int n, long long p, int i, long long stride,
                                                  float step) {
    if (i == 0) return __fdiv_rn(__fsub_rn(s[p + stride], s[p]), step);
    if (i == n - 1) return __fdiv_rn(__fsub_rn(s[p], s[p - stride]), step);
    return __fdiv_rn(__fsub_rn(s[p + stride], s[p - stride]), __fmul_rn(2.0f, step));
}

// one thread per lattice point writes the vertices of its crossed edges, first[p] onwards, in type order
__global__ void iso_vertices_kernel(const float* __restrict__ s, const Lattice l, float iso, const uint8_t* __restrict__ mask,
                                    const uint32_t* __restrict__ first, float* __restrict__ vertices,
                                    float* __restrict__ normals) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int n = l.n;
    if (p >= (long long)n * n * n) return;
    const unsigned m = mask[p];
    if (m == 0) return;
    const int i0[3] = {(int)(p % n), (int)((p / n) % n), (int)(p / ((long long)n * n))};
    const long long stride[3] = {1, n, (long long)n * n};
    const float s0 = s[p];
    float p0[3], g0[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        p0[a] = lattice_coord(l, a, i0[a]);
        g0[a] = lattice_gradient(s, n, p, i0[a], stride[a], l.step[a]);
    }
    size_t v = first[p];
    for (int t = 0; t < 7; ++t) {
        if (!((m >> t) & 1u)) continue;
        const int d[3] = {kEdge[t][0], kEdge[t][1], kEdge[t][2]};
        const long long q = p + d[0] + (long long)n * (d[1] + (long long)n * d[2]);
        const float s1 = s[q];
        float w = __fdiv_rn(__fsub_rn(iso, s0), __fsub_rn(s1, s0));
        if (!finite_f(w)) w = 0.5f;
        float g[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float p1 = lattice_coord(l, a, i0[a] + d[a]);
            vertices[3 * v + a] = __fadd_rn(p0[a], __fmul_rn(w, __fsub_rn(p1, p0[a])));
            const float g1 = lattice_gradient(s, n, q, i0[a] + d[a], stride[a], l.step[a]);
            g[a] = __fadd_rn(g0[a], __fmul_rn(w, __fsub_rn(g1, g0[a])));
        }
        const float len = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(g[0], g[0]), __fmul_rn(g[1], g[1])), __fmul_rn(g[2], g[2])));
        const bool ok = finite_f(len) && len > 0.f;
#pragma unroll
        for (int a = 0; a < 3; ++a) normals[3 * v + a] = ok ? -__fdiv_rn(g[a], len) : 0.f;
        ++v;
    }
}

// id of the vertex on the edge from corner `from` to corner `to` (offset codes, from a subset of to) of the cube at `base`
__device__ __forceinline__ int edge_vertex(const uint8_t* __restrict__ mask, const uint32_t* __restrict__ first, int n,
                                           long long base, int from, int to) {
    const long long p = base + (from & 1) + (long long)n * (((from >> 1) & 1) + (long long)n * (from >> 2));
    const int type = kTypeOfCode[to ^ from];
    return (int)(first[p] + __popc(mask[p] & ((1u << type) - 1u)));
}

// one thread per cube writes its triangles, tfirst[c] onwards, tetrahedron by tetrahedron
__global__ void iso_triangles_kernel(const float* __restrict__ s, int n, float iso, const uint8_t* __restrict__ mask,
                                     const uint32_t* __restrict__ first, const uint8_t* __restrict__ count,
                                     const uint32_t* __restrict__ tfirst, int* __restrict__ triangles) {
    const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int m = n - 1;
    if (c >= (long long)m * m * m) return;
    if (count[c] == 0) return;
    const int cx = (int)(c % m), cy = (int)((c / m) % m), cz = (int)(c / ((long long)m * m));
    const long long base = cx + (long long)n * (cy + (long long)n * cz);
    const unsigned bits = cube_inside_bits(s, n, iso, base);
    size_t t = tfirst[c];
    for (int perm = 0; perm < 6; ++perm) {
        int code[4];
        const unsigned cs = tet_case(bits, perm, code);
        const int k = __popc(cs);
        if (k == 0 || k == 4) continue;
        int q[4], len;
        if (k == 2) {
            int in[2], out[2], ni = 0, no = 0;
            for (int i = 0; i < 4; ++i) {
                if ((cs >> i) & 1u) in[ni++] = i; else out[no++] = i;
            }
            const int pairs[4][2] = {{in[0], out[0]}, {in[0], out[1]}, {in[1], out[1]}, {in[1], out[0]}};
            for (int e = 0; e < 4; ++e) {
                const int a = min(pairs[e][0], pairs[e][1]), b = max(pairs[e][0], pairs[e][1]);
                q[e] = edge_vertex(mask, first, n, base, code[a], code[b]);
            }
            len = 4;
        } else {
            const unsigned odd_bits = k == 1 ? cs : (~cs & 0xfu);
            const int odd = __ffs(odd_bits) - 1;
            len = 0;
            for (int j = 0; j < 4; ++j) {
                if (j == odd) continue;
                const int a = min(odd, j), b = max(odd, j);
                q[len++] = edge_vertex(mask, first, n, base, code[a], code[b]);
            }
            q[3] = 0;
        }
        const bool flip = (((kFlipEven >> cs) ^ (kPermOdd >> perm)) & 1u) != 0;
        if (flip) {                                            // reverse the cycle
            const int a = q[0], b = q[1];
            if (len == 3) { q[0] = q[2]; q[2] = a; }
            else { q[0] = q[3]; q[3] = a; q[1] = q[2]; q[2] = b; }
        }
        int lowest = 0;
        for (int e = 1; e < len; ++e) if (q[e] < q[lowest]) lowest = e;
        int r[4];
        for (int e = 0; e < 4; ++e) r[e] = q[(lowest + e) % len];
        triangles[3 * t + 0] = r[0]; triangles[3 * t + 1] = r[1]; triangles[3 * t + 2] = r[2];
        ++t;
        if (len == 4) {
            triangles[3 * t + 0] = r[0]; triangles[3 * t + 1] = r[2]; triangles[3 * t + 2] = r[3];
            ++t;
        }
    }
}

// ---- exclusive scan of N byte-sized counts into uint32: reduce per tile, scan the tile sums in one block, scan per tile ----
// A tile is kScanTile items: kScanPasses passes of 256 threads x 4 consecutive items (one 4-byte load, one 16-byte store per
// thread).  POPC: the item is a bit mask and counts as its number of set bits.  512^3 items are 32768 tiles, which the
// one-block middle level takes as 32 consecutive sums per thread; every level runs at every size above one tile.
constexpr int kScanPasses = 4;
constexpr int kScanTile = kBs * 4 * kScanPasses;

template <bool POPC>
__device__ __forceinline__ void load4(const uint8_t* __restrict__ in, long long i, long long N, unsigned v[4]) {
    uint32_t w = 0;
    if (i + 4 <= N) w = *reinterpret_cast<const uint32_t*>(in + i);
    else
        for (int k = 0; k < 4; ++k) if (i + k < N) w |= (uint32_t)in[i + k] << (8 * k);
    for (int k = 0; k < 4; ++k) {
        const unsigned b = (w >> (8 * k)) & 0xffu;
        v[k] = POPC ? (unsigned)__popc(b) : b;
    }
}

// inclusive scan of one value per thread over the block; *total = the block's sum.  tmp: blockDim.x / 64 words of LDS
__device__ __forceinline__ unsigned block_inclusive_scan(unsigned x, unsigned* tmp, unsigned* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    if (lane == 63) tmp[wave] = x;
    __syncthreads();
    unsigned before = 0, all = 0;
    for (int w = 0; w < waves; ++w) {
        const unsigned s = tmp[w];
        if (w < wave) before += s;
        all += s;
    }
    __syncthreads();                                           // tmp is free again
    *total = all;
    return x + before;
}

template <bool POPC>
__global__ __launch_bounds__(kBs) void scan_reduce_kernel(const uint8_t* __restrict__ in, long long N, uint32_t* __restrict__ sums) {
    __shared__ unsigned tmp[kBs / 64];
    const long long tile = (long long)blockIdx.x * kScanTile;
    unsigned acc = 0;
    for (int pass = 0; pass < kScanPasses; ++pass) {
        const long long i = tile + ((long long)pass * kBs + threadIdx.x) * 4;
        if (i < N) {
            unsigned v[4];
            load4<POPC>(in, i, N, v);
            acc += v[0] + v[1] + v[2] + v[3];
        }
    }
    unsigned total;
    block_inclusive_scan(acc, tmp, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// in place: sums[0..nb) -> their exclusive scan; *total = the sum of all.  One block.
__global__ __launch_bounds__(1024) void scan_sums_kernel(uint32_t* __restrict__ sums, int nb, uint32_t* __restrict__ total_out) {
    __shared__ unsigned tmp[1024 / 64];
    const int per = (nb + 1023) / 1024;
    const int begin = min((int)threadIdx.x * per, nb), end = min(begin + per, nb);
    unsigned acc = 0;
    for (int i = begin; i < end; ++i) acc += sums[i];
    unsigned total;
    unsigned run = block_inclusive_scan(acc, tmp, &total) - acc;
    for (int i = begin; i < end; ++i) {
        const unsigned v = sums[i];
        sums[i] = run;
        run += v;
    }
    if (threadIdx.x == 0) *total_out = total;
}

template <bool POPC>
__global__ __launch_bounds__(kBs) void scan_apply_kernel(const uint8_t* __restrict__ in, long long N, const uint32_t* __restrict__ sums,
                                                         uint32_t* __restrict__ out) {
    __shared__ unsigned tmp[kBs / 64];
    const long long tile = (long long)blockIdx.x * kScanTile;
    unsigned carry = sums[blockIdx.x];
    for (int pass = 0; pass < kScanPasses; ++pass) {            // uniform trip count: the barriers inside are reached by all
        const long long i = tile + ((long long)pass * kBs + threadIdx.x) * 4;
        unsigned v[4] = {0, 0, 0, 0};
        if (i < N) load4<POPC>(in, i, N, v);
        const unsigned mine = v[0] + v[1] + v[2] + v[3];
        unsigned total;
        const unsigned x0 = carry + block_inclusive_scan(mine, tmp, &total) - mine;
        const unsigned x1 = x0 + v[0], x2 = x1 + v[1], x3 = x2 + v[2];
        if (i + 4 <= N) *reinterpret_cast<uint4*>(out + i) = make_uint4(x0, x1, x2, x3);
        else {
            if (i < N) out[i] = x0;
            if (i + 1 < N) out[i + 1] = x1;
            if (i + 2 < N) out[i + 2] = x2;
        }
        carry += total;
    }
}

// out[i] = sum of in[0..i) (POPC: of their bit counts), *total_dev = the sum of all N; sums: scratch of ceil(N / kScanTile) words
template <bool POPC>
void launch_scan(const uint8_t* in, long long N, uint32_t* sums, uint32_t* out, uint32_t* total_dev, hipStream_t stream) {
    const int nb = (int)((N + kScanTile - 1) / kScanTile);
    hipLaunchKernelGGL(scan_reduce_kernel<POPC>, dim3(nb), dim3(kBs), 0, stream, in, N, sums);
    hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(1024), 0, stream, sums, nb, total_dev);
    hipLaunchKernelGGL(scan_apply_kernel<POPC>, dim3(nb), dim3(kBs), 0, stream, in, N, sums, out);
}

int read_total(nerf_ctx* c, const uint32_t* dev, const char* what, long long* out) {
    uint32_t host = 0;
    HIP_OK(hipMemcpyAsync(&host, dev, sizeof host, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    if (host > (uint32_t)INT32_MAX) return fail("isosurface: %u %s do not fit int32", host, what);
    *out = host;
    return 0;
}

}  // namespace

// the scan above for the other translation units (cull_kernels.hip's bit mask): POPC items
size_t scan_sums_words(long long N) { return (size_t)((N + kScanTile - 1) / kScanTile); }
void launch_scan_popc(const uint8_t* in, long long N, uint32_t* sums, uint32_t* out, uint32_t* total_dev, hipStream_t stream) {
    launch_scan<true>(in, N, sums, out, total_dev, stream);
}

}  // namespace nerf

using namespace nerf;

extern "C" {

int nerf_isosurface(nerf_ctx* c, const float* sigma, int32_t n, const float* lo3, const float* hi3, float iso,
                    int64_t* n_vertices, int64_t* n_triangles, int mem) {
    ENTER(c);
    if (!sigma || !lo3 || !hi3 || !n_vertices || !n_triangles) return fail("NULL argument");
    if (int r = lattice_n_ok("isosurface", n)) return r;
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(lo3[a]) || !std::isfinite(hi3[a]) || !(lo3[a] < hi3[a]))
            return fail("isosurface needs finite lo < hi on every axis (axis %d: lo %g, hi %g)", a, lo3[a], hi3[a]);
    if (!std::isfinite(iso)) return fail("isosurface: iso must be finite (got %g)", iso);
    c->mesh_on = false;                                        // a call that fails leaves no mesh behind
    const long long points = (long long)n * n * n, cubes = (long long)(n - 1) * (n - 1) * (n - 1);
    Staging st(c, mem);      // (no outputs: the mesh stays in the ctx until nerf_isosurface_fetch)
    const float* s = st.in(c->b_mesh_sigma, sigma, (size_t)points * 4);
    if (st.err) return st.err;
    const size_t tiles = (size_t)((points + kScanTile - 1) / kScanTile);
    if (int r = ensure(c, c->b_mesh_mask, (size_t)points)) return r;
    if (int r = ensure(c, c->b_mesh_first, (size_t)points * 4)) return r;
    if (int r = ensure(c, c->b_mesh_count, (size_t)cubes)) return r;
    if (int r = ensure(c, c->b_mesh_tfirst, (size_t)cubes * 4)) return r;
    if (int r = ensure(c, c->b_mesh_sums, (tiles + 2) * 4)) return r;
    uint8_t *mask = (uint8_t*)c->b_mesh_mask.p, *count = (uint8_t*)c->b_mesh_count.p;
    uint32_t *first = (uint32_t*)c->b_mesh_first.p, *tfirst = (uint32_t*)c->b_mesh_tfirst.p;
    uint32_t *sums = (uint32_t*)c->b_mesh_sums.p, *totals = sums + tiles;
    const Lattice l = make_lattice(lo3, hi3, n);

    hipLaunchKernelGGL(iso_point_mask_kernel, dim3(blocks_for(points)), dim3(kBs), 0, c->stream, s, n, iso, mask);
    launch_scan<true>(mask, points, sums, first, totals, c->stream);
    hipLaunchKernelGGL(iso_cube_count_kernel, dim3(blocks_for(cubes)), dim3(kBs), 0, c->stream, s, n, iso, count);
    launch_scan<false>(count, cubes, sums, tfirst, totals + 1, c->stream);
    HIP_OK(hipGetLastError());
    long long V = 0, T = 0;
    if (int r = read_total(c, totals, "vertices", &V)) return r;
    if (int r = read_total(c, totals + 1, "triangles", &T)) return r;
    if (V > 0) {
        if (int r = ensure(c, c->b_mesh_v, (size_t)V * 12)) return r;
        if (int r = ensure(c, c->b_mesh_n, (size_t)V * 12)) return r;
        hipLaunchKernelGGL(iso_vertices_kernel, dim3(blocks_for(points)), dim3(kBs), 0, c->stream, s, l, iso, mask, first,
                           (float*)c->b_mesh_v.p, (float*)c->b_mesh_n.p);
    }
    if (T > 0) {
        if (int r = ensure(c, c->b_mesh_t, (size_t)T * 12)) return r;
        hipLaunchKernelGGL(iso_triangles_kernel, dim3(blocks_for(cubes)), dim3(kBs), 0, c->stream, s, n, iso, mask, first, count,
                           tfirst, (int*)c->b_mesh_t.p);
    }
    HIP_OK(hipGetLastError());
    if (int r = st.finish()) return r;
    c->mesh_V = V; c->mesh_T = T;
    c->mesh_on = true;
    *n_vertices = V; *n_triangles = T;
    return 0;
}

int nerf_isosurface_fetch(nerf_ctx* c, float* vertices, float* normals, int32_t* triangles, int mem) {
    ENTER(c);
    if (!c->mesh_on) return fail("no pending mesh: call nerf_isosurface first");
    if ((c->mesh_V > 0 && !vertices) || (c->mesh_T > 0 && !triangles)) return fail("NULL argument");
    if (c->mesh_V > 0) {
        if (int r = copy_to_caller(c, vertices, c->b_mesh_v.p, (size_t)c->mesh_V * 12, mem)) return r;
        if (normals) if (int r = copy_to_caller(c, normals, c->b_mesh_n.p, (size_t)c->mesh_V * 12, mem)) return r;
    }
    if (c->mesh_T > 0) if (int r = copy_to_caller(c, triangles, c->b_mesh_t.p, (size_t)c->mesh_T * 12, mem)) return r;
    if (mem == NERF_MEM_HOST) HIP_OK(hipStreamSynchronize(c->stream));
    return 0;
}

}  // extern "C"
