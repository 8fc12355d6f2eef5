// weight_tables.hip -- from a weight blob to the kernels' operand streams, host half: the shape of the blob (layer_dims), the
// map between blobs of different octave counts (blob_expand_index, aim_gather) and every gather table of a config
// (build_stream_tables).  Host code only; the device half is aux_kernels.hip::launch_repack.
#include "nerf_kernels.h"

#include <string.h>

#include <algorithm>

namespace nerf {

int layer_dims(int lx, int ld, int n_angles, int dims[12][2]) {
    const int xd = 3 + 6 * lx;                                  // src/NeRF.py:312
    const int kd = 256 + 2 * ld * (n_angles + 1);               // [hidden, dir_enc], src/NeRF.py:313-314
    const int with_dirs[11][2] = {{xd, 256}, {256, 256}, {256, 256}, {256, 256}, {xd + 256, 256}, {256, 256},
                                  {256, 256}, {256, 256}, {kd, 128}, {128, 3}, {kd, 1}};
    // get_network_only_xyz (src/NeRF.py:248-288): ..., 8: 256 -> 256, 9: 256 -> 128, 10: 128 -> 3, 11: 256 -> 1
    const int xyz_only[12][2] = {{xd, 256}, {256, 256}, {256, 256}, {256, 256}, {xd + 256, 256}, {256, 256},
                                 {256, 256}, {256, 256}, {256, 256}, {256, 128}, {128, 3}, {256, 1}};
    const int n = n_angles == 0 ? 12 : 11;
    for (int l = 0; l < n; ++l) {
        dims[l][0] = n_angles == 0 ? xyz_only[l][0] : with_dirs[l][0];
        dims[l][1] = n_angles == 0 ? xyz_only[l][1] : with_dirs[l][1];
    }
    return n;
}

size_t blob_floats(int lx, int ld, int n_angles) {
    int dims[12][2];
    const int n = layer_dims(lx, ld, n_angles, dims);
    size_t s = 0;
    for (int l = 0; l < n; ++l) s += (size_t)dims[l][0] * dims[l][1] + dims[l][1];
    return s;
}

void blob_expand_index(int lx, int ld, int n_angles, int32_t* idx, int layout_lx) {
    int wide[12][2], dims[12][2];
    const int n = layer_dims(layout_lx, kLd, n_angles, wide);
    layer_dims(lx, ld, n_angles, dims);
    const int xd_layout = 3 + 6 * layout_lx;
    // xyz encoding row of the (layout_lx) layout -> row of the (lx) layout: per component [x, sin0, cos0, sin1, cos1, ...]
    auto xyz_row = [&](int r) {
        const int c = r / (1 + 2 * layout_lx), j = r % (1 + 2 * layout_lx);
        if (j == 0) return c * (1 + 2 * lx);
        const int k = (j - 1) / 2, h = (j - 1) % 2;
        return k < lx ? c * (1 + 2 * lx) + 1 + 2 * k + h : -1;
    };
    // direction encoding row: per component [sin0, cos0, sin1, cos1, ...] (src/UtilsNeuralRadianceField.py:52-65)
    auto dir_row = [&](int r) {
        const int c = r / (2 * kLd), j = r % (2 * kLd), k = j / 2, h = j % 2;
        return k < ld ? c * 2 * ld + 2 * k + h : -1;
    };
    size_t src = 0, dst = 0;
    for (int l = 0; l < n; ++l) {
        for (int r = 0; r < wide[l][0]; ++r) {
            int rs = r;
            if (l == 0) rs = xyz_row(r);
            else if (l == 4) rs = r < xd_layout ? xyz_row(r) : 3 + 6 * lx + (r - xd_layout);
            else if (n_angles != 0 && (l == 8 || l == 10)) rs = r < kHidden ? r : (dir_row(r - kHidden) < 0 ? -1 : kHidden + dir_row(r - kHidden));
            for (int f = 0; f < wide[l][1]; ++f)
                idx[dst++] = rs < 0 ? 0 : (int32_t)(src + (size_t)rs * dims[l][1] + f + 1);
        }
        src += (size_t)dims[l][0] * dims[l][1];
        for (int f = 0; f < wide[l][1]; ++f) idx[dst++] = (int32_t)(src + f + 1);
        src += dims[l][1];
    }
}

void aim_gather(int lx, int ld, int n_angles, int32_t* idx, size_t n, bool f16) {
    const int L = pe_layout_lx(lx);
    if (lx == L && ld == kLd) return;
    std::vector<int32_t> map(blob_floats(L, kLd, n_angles));
    blob_expand_index(lx, ld, n_angles, map.data(), L);
    for (size_t i = 0; i < n; ++i) {
        const int32_t t = idx[i];
        if (!t) continue;
        const int32_t m = map[(f16 ? t >> 1 : t) - 1];
        idx[i] = m == 0 ? 0 : f16 ? 2 * m + (t & 1) : m;
    }
}

void build_scale_table(int lx, int ld, int n_angles, const float* w_xyz, const float* w_dir, std::vector<float>& scale) {
    int dims[12][2];
    const int n = layer_dims(lx, ld, n_angles, dims);
    scale.assign(blob_floats(lx, ld, n_angles), 1.f);
    const int xd = 3 + 6 * lx, dd = 2 * ld * (n_angles + 1);
    size_t off = 0;
    for (int l = 0; l < n; ++l) {
        // the rows of layer l that an encoding enters, in blob_expand_index's row order: xyz [x, sin0, cos0, ...] per
        // component at the top of layers 0 and 4, direction [sin0, cos0, ...] per component below the 256 hidden rows of 8, 10
        const bool xyz_rows = l == 0 || l == 4, dir_rows = n_angles != 0 && (l == 8 || l == 10);
        for (int r = 0; r < (xyz_rows ? xd : 0); ++r) {
            const int j = r % (1 + 2 * lx);
            if (j == 0) continue;                    // the pass-through component
            std::fill_n(scale.begin() + off + (size_t)r * dims[l][1], dims[l][1], w_xyz[(j - 1) / 2]);
        }
        for (int r = 0; r < (dir_rows ? dd : 0); ++r)
            std::fill_n(scale.begin() + off + (size_t)(kHidden + r) * dims[l][1], dims[l][1], w_dir[(r % (2 * ld)) / 2]);
        off += (size_t)dims[l][0] * dims[l][1] + dims[l][1];
    }
}

void build_stream_tables(int lx, int ld, int n_angles, StreamTables& t) {
    StreamDesc d[2][kStreamKinds];
    for (int w = 0; w < 2; ++w) render_streams(lx, n_angles, w, d[w]);
    for (auto& c : t.cst) c.clear();
    for (int k = 0; k < kStreamKinds; ++k) {
        const size_t bytes = std::max(d[0][k].bytes, d[1][k].bytes);
        const bool f16 = d[0][k].elem != kElemF32;
        t.stream[k].clear();
        if (!bytes || d[0][k].table != k) continue;
        t.stream[k].assign(bytes / (f16 ? 2 : 4), 0);
        std::vector<int32_t> ci(kConstFloats, 0);
        if (build_stream_gather(lx, n_angles, (StreamKind)k, t.stream[k].data(), ci.data())) {
            aim_gather(lx, ld, n_angles, ci.data(), ci.size(), false);
            t.cst[d[0][k].cst] = ci;
        }
        aim_gather(lx, ld, n_angles, t.stream[k].data(), t.stream[k].size(), f16);
    }
}

}  // namespace nerf

// Debug entry (not part of include/nerf_mi355.h; host only, no device is touched): the 64-bit FNV-1a hash of the gather table
// of stream kind `kind` of network `which` of an (lx, ld, n_angles) config, over its int32 entries' bytes in little-endian
// order -- the hash tests/golden/stream_table_hashes*.txt record, the kind by the name those files give it.  0: that network
// keeps no such stream of its own; ~0: no kind of that name.
extern "C" unsigned long long nerf_debug_stream_table_hash(int lx, int ld, int n_angles, int which, const char* kind_name) {
    using namespace nerf;
    static const char* kNames[kStreamKinds] = {"f16x3", "f16hi", "bf16x3", "f16x3sig", "bf16x3sig", "fp32", "f16x3skip"};
    static_assert(kF16x3 == 0 && kF16Hi == 1 && kBf16x3 == 2 && kF16x3Sig == 3 && kBf16x3Sig == 4 && kFp32 == 5 && kF16x3Skip == 6,
                  "kNames follows StreamKind");
    int kind = -1;
    for (int k = 0; k < kStreamKinds; ++k) if (kind_name && !strcmp(kind_name, kNames[k])) kind = k;
    if (kind < 0) return ~0ull;
    if (which != 0 && which != 1) return 0;
    StreamDesc d[kStreamKinds];
    render_streams(lx, n_angles, which, d);
    if (!d[kind].bytes || d[kind].table != kind) return 0;
    StreamTables t;
    build_stream_tables(lx, ld, n_angles, t);
    const size_t n = d[kind].bytes / (d[kind].elem != kElemF32 ? 2 : 4);
    unsigned long long h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < n; ++i)
        for (int b = 0; b < 4; ++b) { h ^= ((uint32_t)t.stream[kind][i] >> (8 * b)) & 0xffu; h *= 0x100000001b3ull; }
    return h;
}
