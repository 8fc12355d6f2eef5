// Host-side packers and gather-table builders under AddressSanitizer (CPU only: nothing here touches a GPU).
// It walks the render path's stream table (nerf_kernels.h::render_streams): every output buffer has exactly the size the
// table lists, so a write past it is reported.
//   hipcc -fsanitize=address -fno-gpu-sanitize -O1 -g --offload-arch=gfx950 -std=c++17 -I. tools/pack_asan_test.cpp \
//         mlp_fp32.hip mlp_f16x3.hip mlp_f16x3_wide.hip mlp_bf16x3.hip mlp_bf16x3_wide.hip mlp_bwd_f16x3.hip \
//         -o /tmp/pack_asan && /tmp/pack_asan
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "nerf_kernels.h"
using namespace nerf;
int main() {
    double s = 0;
    for (int n_angles : {2, 1, 0})
        for (int lx : {5, 8}) {
            // floats of the blob the packers of this build read: the (pe_layout_lx, kLd) layout
            const int xd = 3 + 6 * pe_layout_lx(lx), kd = 256 + 8 * (n_angles + 1);
            const size_t nblob = n_angles == 0 ? size_t(xd + 1) * 256 + 6 * 257 * 256 + size_t(xd + 257) * 256 + 257 * 256 + 257 * 128 + 129 * 3 + 257
                                               : size_t(xd + 1) * 256 + 6 * 257 * 256 + size_t(xd + 257) * 256 + size_t(kd + 1) * 128 + 129 * 3 + kd + 1;
            std::vector<float> blob(nblob);
            for (size_t i = 0; i < blob.size(); ++i) blob[i] = (float)rand() / RAND_MAX - 0.5f;
            for (int which : {0, 1}) {
                StreamDesc d[kStreamKinds];
                render_streams(lx, n_angles, which, d);
                for (int k = 0; k < kStreamKinds; ++k) {
                    if (!d[k].bytes) continue;
                    std::vector<char> st(d[k].bytes);
                    std::vector<float> cs(kConstFloats);
                    d[k].pack(blob.data(), n_angles, st.data(), cs.data());
                    for (char v : st) s += v;
                    if (d[k].table != k || k == kFp32) continue;      // (the fp32 table is the packer itself, run on an index blob)
                    std::vector<int32_t> si(d[k].bytes / 2), ci(kConstFloats);
                    build_stream_gather(lx, n_angles, (StreamKind)k, si.data(), ci.data());
                    for (auto v : si) if (v < 0 || (size_t)(v >> 1) > nblob) { printf("gather index out of the blob\n"); return 1; }
                    for (auto v : ci) if (v < 0 || (size_t)v > nblob) { printf("const index out of the blob\n"); return 1; }
                }
            }
            // the trainer's backward stream (not a render stream: no table entry)
            for (bool hi_only : {false, true})
                for (bool dx : {false, true}) {
                    std::vector<int32_t> bi(kBwdStreamBytes / 2);
                    build_bwd_gather(n_angles, dx, hi_only, bi.data(), xd);
                    for (auto v : bi) if (v < 0 || (size_t)(v >> 1) > nblob) { printf("bwd gather index out of the blob\n"); return 1; }
                    s += bi[17];
                }
        }
    printf("ok %f\n", s);
    return 0;
}
