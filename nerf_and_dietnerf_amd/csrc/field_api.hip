// field_api.hip -- field queries: the entry points that run a network on points the library makes itself, chunk by chunk, and
// rework the raw rows -- the occupancy bake (with the grid's setter and getter), the density and radiance lattices, the vertex
// colours (include/nerf_mi355.h has the rules).  One chunk loop around eval_points; the fills and drains: field_kernels.hip.
#include <algorithm>
#include <cmath>
#include <vector>

#include "field_device.h"
#include "nerf_ctx.h"

using namespace nerf;

namespace {

constexpr long long kMeshChunk = 1LL << 20;   // points per pass through the network
const char* const kGridNeedsBox = "an occupancy grid needs a scene box (nerf_ctx_set_scene_box)";

int grid_resolution_ok(int R) {
    return R < 4 || R > 256 || R % 4 ? fail("occupancy grid resolution must be a multiple of 4 in [4, 256] (got %d)", R) : 0;
}

// what every query refuses, in the order every one of them always has: which, then its own refusals, then missing weights
template <class Own>
int query_ok(const nerf_ctx* c, int which, Own own) {
    if (which != 0 && which != 1) return fail("which must be 0 (coarse) or 1 (fine)");
    if (int r = own()) return r;
    return c->net[which].loaded ? 0 : fail("network %d has no weights loaded", which);
}

// One pass through the network: items [begin, begin + m), the buffers of their points, view directions (NULL: the network takes
// none) and raw rows, and the points the network reads -- xyz, unless fill names device points the caller already has.
struct Chunk { long long begin, m; float *xyz, *view, *raw; const float* points; };

// Network `which` on `total` items of `per` points each, `chunk` items per pass, on the ctx stream: fill(k) writes the points
// (and view directions) of chunk k, drain(k) consumes its (m * per, 4) raw rows.
template <class Fill, class Drain>
int for_each_chunk(nerf_ctx* c, int which, long long total, long long chunk, int per, Fill fill, Drain drain) {
    const size_t pts = (size_t)std::min(total, chunk) * per;
    if (int r = ensure(c, c->b_in0, pts * 12)) return r;
    if (int r = ensure(c, c->b_in1, pts * 12)) return r;
    if (int r = ensure(c, c->b_raw, pts * 16)) return r;
    Chunk k = {0, 0, (float*)c->b_in0.p, c->cfg.n_angles != 0 ? (float*)c->b_in1.p : nullptr, (float*)c->b_raw.p, nullptr};
    for (; k.begin < total; k.begin += chunk) {
        k.m = std::min(chunk, total - k.begin);
        k.points = k.xyz;
        if (int r = fill(k)) return r;
        if (int r = eval_points(c, which, k.points, k.view, k.m * per, k.raw)) return r;
        if (int r = drain(k)) return r;
    }
    HIP_OK(hipGetLastError());
    return 0;
}

// The n^3 lattice of the scene box (field_device.h) -> result (n^3, channels): 1 the raw sigma, 4 the radiance volume's texel.
// Every point sees along view_dir3 (NULL: (0, 0, 1), the bake's), or along the ray of camera cam through it.
int lattice_query(nerf_ctx* c, int which, const char* what, int n, const float* view_dir3, const float* cam, int channels,
                  float* result, int mem) {
    ENTER(c);
    if (!result) return fail("NULL argument");
    if (int r = query_ok(c, which, [&] {
            if (view_dir3 && cam) return fail("%s: give view_dir or camera, not both", what);
            if (!c->box_on) return fail("a %s needs a scene box (nerf_ctx_set_scene_box)", what);
            if (int r = lattice_n_ok(what, n)) return r;
            if (cam && c->ray_space == NERF_RAYS_NDC)
                return fail("%s: camera is refused while the ray space is NDC (the scene box is not in world space)", what);
            return 0;
        })) return r;
    const float up[3] = {0.f, 0.f, 1.f}, *vd = view_dir3 ? view_dir3 : up;
    const long long points = (long long)n * n * n;
    Staging st(c, mem);
    float* out = st.out(c->b_lattice, result, (size_t)points * channels * 4);
    if (st.err) return st.err;
    const int r = for_each_chunk(c, which, points, kMeshChunk, 1,
        [&](Chunk& k) {
            const bool per_point = cam && k.view;
            launch_lattice_points(c->box, n, k.begin, k.m, vd, k.xyz, per_point ? nullptr : k.view, c->stream);
            if (per_point) launch_camera_view(cam, k.xyz, k.m, k.view, c->stream);
            return 0;
        },
        [&](const Chunk& k) {
            (channels == 4 ? launch_raw_rgba : launch_raw_sigma)(k.raw, k.m, out + channels * k.begin, c->stream);
            return 0;
        });
    return r ? r : st.finish();
}

}  // namespace

extern "C" {

int nerf_ctx_set_occupancy_grid(nerf_ctx* c, const uint32_t* bits, int32_t R) {
    ENTER(c);
    if (!bits && R == 0) { c->grid_R = 0; return 0; }
    if (!bits) return fail("occupancy grid: bits is NULL (NULL, 0 clears the grid)");
    if (!c->box_on) return fail("%s", kGridNeedsBox);
    if (int r = grid_resolution_ok(R)) return r;
    const size_t bytes = (size_t)R * R * R / 8;
    c->grid_R = 0;
    if (int r = ensure(c, c->b_grid[0], bytes)) return r;
    HIP_OK(hipMemcpyAsync(c->b_grid[0].p, bits, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));          // the caller's array is free again
    c->grid_cur = 0; c->grid_R = R;
    return 0;
}

int nerf_ctx_get_occupancy_grid(nerf_ctx* c, uint32_t* bits, int32_t* R) {
    ENTER(c);
    if (!R) return fail("NULL argument");
    *R = c->grid_R;
    if (!bits || c->grid_R == 0) return 0;
    const size_t bytes = (size_t)c->grid_R * c->grid_R * c->grid_R / 8;
    HIP_OK(hipMemcpyAsync(bits, c->b_grid[c->grid_cur].p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    return 0;
}

int nerf_occupancy_bake(nerf_ctx* c, int which, int32_t R, float sigma_threshold, int32_t samples_per_cell, int32_t dilate,
                        uint64_t seed, int64_t* n_occupied) {
    ENTER(c);
    const int spc = samples_per_cell;
    if (int r = query_ok(c, which, [&] {
            if (!c->box_on) return fail("%s", kGridNeedsBox);
            if (int r = grid_resolution_ok(R)) return r;
            if (!std::isfinite(sigma_threshold) || !(sigma_threshold > 0.f))
                return fail("occupancy grid: sigma_threshold must be finite and > 0 (got %g)", sigma_threshold);
            if (spc < 1 || spc > 8) return fail("occupancy grid: samples_per_cell must be in 1..8 (got %d)", spc);
            if (dilate < 0 || dilate > 2) return fail("occupancy grid: dilate must be 0, 1 or 2 (got %d)", dilate);
            return 0;
        })) return r;
    const long long cells = (long long)R * R * R;                 // a multiple of 64
    const size_t bytes = (size_t)cells / 8;
    c->grid_R = 0;                                                // a bake that fails leaves no grid behind
    if (int r = ensure(c, c->b_grid[0], bytes)) return r;
    if (int r = ensure(c, c->b_grid[1], bytes)) return r;
    if (int r = for_each_chunk(c, which, cells, std::min(cells, (kMeshChunk / spc) & ~63LL), spc,   // whole 64-cell groups
            [&](Chunk& k) { launch_grid_points(c->box, R, k.begin, k.m, spc, seed, k.xyz, k.view, c->stream); return 0; },
            [&](const Chunk& k) {
                launch_grid_threshold(k.raw, k.begin, k.m, spc, sigma_threshold, (uint32_t*)c->b_grid[0].p, c->stream);
                return 0;
            })) return r;
    int cur = 0;
    for (int i = 0; i < dilate; ++i, cur ^= 1)
        launch_grid_dilate((const uint32_t*)c->b_grid[cur].p, (uint32_t*)c->b_grid[cur ^ 1].p, R, c->stream);
    HIP_OK(hipGetLastError());
    if (n_occupied) {
        std::vector<uint32_t> host(bytes / 4);
        HIP_OK(hipMemcpyAsync(host.data(), c->b_grid[cur].p, bytes, hipMemcpyDeviceToHost, c->stream));
        HIP_OK(hipStreamSynchronize(c->stream));
        long long count = 0;
        for (uint32_t w : host) count += __builtin_popcount(w);
        *n_occupied = count;
    }
    c->grid_cur = cur; c->grid_R = R;
    return 0;
}

int nerf_density_lattice(nerf_ctx* c, int which, int32_t n, const float* view_dir3, float* sigma, int mem) {
    return lattice_query(c, which, "density lattice", n, view_dir3, nullptr, 1, sigma, mem);
}

int nerf_radiance_lattice(nerf_ctx* c, int which, int32_t n, const float* view_dir3, const float* camera_c2w16, float* volume,
                          int mem) {
    return lattice_query(c, which, "radiance lattice", n, view_dir3, camera_c2w16, 4, volume, mem);
}

int nerf_sh_radiance_lattice(nerf_ctx* c, int which, int32_t n, int32_t degree, const float* dirs, const float* proj, int32_t D,
                             float* volume, int mem) {
    const char* what = "SH radiance lattice";
    ENTER(c);
    if (!volume) return fail("NULL argument");
    if (int r = query_ok(c, which, [&] {
            if (!c->box_on) return fail("an %s needs a scene box (nerf_ctx_set_scene_box)", what);
            if (int r = lattice_n_ok(what, n)) return r;
            if (degree < 0 || degree > kShMaxDegree) return fail("%s: degree must be in 0..%d (got %d)", what, kShMaxDegree, degree);
            if (D < 1 || D > kShMaxDirs) return fail("%s: D must be in 1..%d (got %d)", what, kShMaxDirs, D);
            if (!dirs || !proj) return fail("%s: %s is NULL", what, dirs ? "proj" : "dirs");
            for (int j = 0; j < D; ++j) {
                const float* d = dirs + 3 * j;
                for (int a = 0; a < 3; ++a)
                    if (!std::isfinite(d[a])) return fail("%s: dirs[%d][%d] is not finite (%g)", what, j, a, d[a]);
            }
            const int K = sh_basis_count(degree);
            for (int k = 0; k < K; ++k)
                for (int j = 0; j < D; ++j)
                    if (!std::isfinite(proj[k * D + j]))
                        return fail("%s: proj[%d][%d] is not finite (%g)", what, k, j, proj[k * D + j]);
            for (int j = 0; j < D; ++j)
                if (dirs[3 * j] == 0.f && dirs[3 * j + 1] == 0.f && dirs[3 * j + 2] == 0.f)
                    return fail("%s: dirs[%d] is the zero vector", what, j);
            return 0;
        })) return r;
    const int K = sh_basis_count(degree), C = sh_texel_floats(degree);
    const long long points = (long long)n * n * n;
    // the call's table, directions then projection, in the ctx's device buffer; the caller's arrays are free again after it
    if (int r = ensure(c, c->b_sh_table, (size_t)(3 + sh_basis_count(kShMaxDegree)) * kShMaxDirs * 4)) return r;   // the largest
    float* table = (float*)c->b_sh_table.p;
    HIP_OK(hipMemcpyAsync(table, dirs, (size_t)D * 12, hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipMemcpyAsync(table + 3 * D, proj, (size_t)K * D * 4, hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    Staging st(c, mem);
    float* out = st.out(c->b_lattice, volume, (size_t)points * C * 4);
    if (st.err) return st.err;
    const int r = for_each_chunk(c, which, points, std::max(1LL, kMeshChunk / D), D,
        [&](Chunk& k) {
            launch_sh_lattice_points(c->box, n, k.begin, k.m, D, table, k.xyz, k.view, c->stream);
            return 0;
        },
        [&](const Chunk& k) {
            launch_sh_project(k.raw, k.m, degree, D, table + 3 * D, out + (size_t)C * k.begin, c->stream);
            return 0;
        });
    return r ? r : st.finish();
}

int nerf_mesh_colors(nerf_ctx* c, int which, const float* vertices, const float* normals, int64_t V, float* rgb, int mem) {
    ENTER(c);
    if (V < 0) return fail("bad V");
    if (V == 0) return 0;
    if (!vertices || !normals || !rgb) return fail("NULL argument");
    if (int r = query_ok(c, which, [] { return 0; })) return r;
    Staging st(c, mem);      // made anew for every chunk: a host caller's chunk is staged, and leaves, by itself
    float* out = nullptr;
    return for_each_chunk(c, which, V, kMeshChunk, 1,
        [&](Chunk& k) {
            st = Staging(c, mem);
            k.points = st.in(c->b_in0, vertices + 3 * k.begin, (size_t)k.m * 12);
            const float* nrm = st.in(c->b_in2, normals + 3 * k.begin, (size_t)k.m * 12);
            out = st.out(c->b_out[0], rgb + 3 * k.begin, (size_t)k.m * 12);
            if (!st.err && k.view) launch_mesh_view(nrm, k.m, k.view, c->stream);
            return st.err;
        },
        [&](const Chunk& k) { launch_raw_rgb(k.raw, k.m, out, c->stream); return st.finish(); });
}

}  // extern "C"
