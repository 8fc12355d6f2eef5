// Gather-table builders under AddressSanitizer (CPU only: nothing here touches a GPU), and the tables themselves against
// recorded hashes.  It walks the render path's stream table (nerf_kernels.h::render_streams, build_stream_tables) and the
// trainer's backward tables: every table has exactly the size its stream lists, so a write past it is reported; every index
// must lie in the network's own blob; and the 64-bit FNV-1a hash of every table must be the one listed in the file given
// as arguments (tests/golden/stream_table_hashes.txt, recorded from the host packers these tables replaced, and
// tests/golden/stream_table_hashes_rgbskip.txt, the sigma-first stream's).
//   hipcc -fsanitize=address -fno-gpu-sanitize -O1 -g --offload-arch=gfx950 -std=c++17 -I. tools/pack_asan_test.cpp \
//         weight_tables.hip mlp_fp32.hip mlp_f16x3.hip mlp_f16x3_wide.hip mlp_bwd_f16x3.hip -o pack_asan \
//         && ./pack_asan ../../tests/golden/stream_table_hashes.txt ../../tests/golden/stream_table_hashes_rgbskip.txt
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <string>
#include <vector>
#include "nerf_kernels.h"
using namespace nerf;

static std::map<std::string, std::string> g_want;
static int g_bad = 0, g_seen = 0;

// f16: entries 2 * (src + 1) + is_lo, else src + 1
static void check(const std::string& key, const std::vector<int32_t>& v, bool f16, size_t nblob) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (int32_t x : v) {
        if (x < 0 || (size_t)(f16 ? x >> 1 : x) > nblob) { printf("%s: index out of the blob\n", key.c_str()); ++g_bad; return; }
        for (int b = 0; b < 4; ++b) { h ^= ((uint32_t)x >> (8 * b)) & 0xffu; h *= 0x100000001b3ull; }
    }
    char hex[17];
    snprintf(hex, sizeof hex, "%016llx", (unsigned long long)h);
    const auto it = g_want.find(key);
    if (it == g_want.end()) { printf("%s: not in the list\n", key.c_str()); ++g_bad; }
    else if (it->second != hex) { printf("%s: hash %s, recorded %s\n", key.c_str(), hex, it->second.c_str()); ++g_bad; }
    ++g_seen;
}

int main(int argc, char** argv) {
    if (argc < 2) { printf("usage: %s stream_table_hashes.txt [more hash files]\n", argv[0]); return 2; }
    for (int f = 1; f < argc; ++f) {
        std::ifstream in(argv[f]);
        for (std::string line; std::getline(in, line);) {
            const size_t sp = line.rfind(' ');
            if (sp != std::string::npos) g_want[line.substr(0, sp)] = line.substr(sp + 1);
        }
    }
    if (g_want.empty()) { printf("no hashes in %s\n", argv[1]); return 2; }
    static const char* kKind[kStreamKinds] = {"f16x3", "f16hi", "bf16x3", "f16x3sig", "bf16x3sig", "fp32", "f16x3skip"};
    static const char* kBlock[kConstBlocks] = {"cst_fp32", "cst_16"};
    for (int lx : {5, 3, 10, 8})
        for (int ld : {4, 2})
            for (int n_angles : {2, 1, 0}) {
                char cfg[64];
                snprintf(cfg, sizeof cfg, "lx=%d ld=%d na=%d ", lx, ld, n_angles);
                const size_t nblob = blob_floats(lx, ld, n_angles);
                StreamTables t;
                build_stream_tables(lx, ld, n_angles, t);
                for (int which : {0, 1}) {
                    StreamDesc d[kStreamKinds];
                    render_streams(lx, n_angles, which, d);
                    for (int k = 0; k < kStreamKinds; ++k) {
                        if (!d[k].bytes || d[k].table != k) continue;
                        const bool f16 = d[k].elem != kElemF32;
                        std::vector<int32_t> tab(t.stream[k].begin(), t.stream[k].begin() + d[k].bytes / (f16 ? 2 : 4));
                        check(cfg + ("which=" + std::to_string(which) + " " + kKind[k]), tab, f16, nblob);
                    }
                }
                for (int b = 0; b < kConstBlocks; ++b)
                    if (!t.cst[b].empty()) check(std::string(cfg) + kBlock[b], t.cst[b], false, nblob);
                {   // the encoding window's scale table: one float per blob element, whole windowed rows and nothing else
                    const float wx[10] = {.5f, .5f, .5f, .5f, .5f, .5f, .5f, .5f, .5f, .5f}, wd[4] = {.25f, .25f, .25f, .25f};
                    std::vector<float> s;
                    build_scale_table(lx, ld, n_angles, wx, wd, s);
                    size_t nx = 0, nd = 0;
                    for (float v : s) { nx += v == .5f; nd += v == .25f; }
                    const size_t want_x = (size_t)2 * 6 * lx * 256, want_d = n_angles ? (size_t)2 * ld * (n_angles + 1) * (128 + 1) : 0;
                    if (s.size() != nblob || nx != want_x || nd != want_d || nx + nd + (size_t)std::count(s.begin(), s.end(), 1.f) != nblob) {
                        printf("FAIL %sscale table: %zu entries (blob %zu), %zu / %zu xyz, %zu / %zu dir\n", cfg, s.size(), nblob, nx,
                               want_x, nd, want_d);
                        ++g_bad;
                    }
                }
                // the trainer's backward stream (not a render stream: no table entry)
                for (int dx : {0, 1})
                    for (int hi_only : {0, 1}) {
                        std::vector<int32_t> bi(kBwdStreamBytes / 2);
                        build_bwd_gather(n_angles, dx, hi_only, bi.data(), pe_layout_lx(lx));
                        aim_gather(lx, ld, n_angles, bi.data(), bi.size(), true);
                        check(cfg + ("bwd_dx" + std::to_string(dx) + "_hi" + std::to_string(hi_only)), bi, true, nblob);
                    }
            }
    if ((size_t)g_seen != g_want.size()) { printf("%d tables built, %zu recorded\n", g_seen, g_want.size()); ++g_bad; }
    printf("%s: %d tables, %d mismatches\n", g_bad ? "FAILED" : "ok", g_seen, g_bad);
    return g_bad ? 1 : 0;
}
