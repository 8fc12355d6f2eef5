"""Cost of the encoding geometry (n_pos_enc_dim_xyz Lx, n_pos_enc_view_dir Ld): rays/s of the render path at 256 x 256,
64 + 128 samples, in each precision (the wide-PE (10, 4) network: f16x3 and f16 only), and the 4096-ray train step under
both policies, for the default (5, 4) network, networks with fewer octaves and the original paper's (10, 4).  All contexts live in one process and are measured in alternation (round r times every
configuration once), so device clocks and neighbours weigh on all of them alike; the median over the rounds is reported.

Usage: python tools/encoding_geometry_bench.py [rounds] [steps per measurement] > result.json"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import nerf_and_dietnerf_amd as N
from oracle import nerf_oracle as O

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
GEOMS = [(5, 4), (5, 2), (3, 4), (1, 1), (10, 4)]      # (10, 4): the wide-PE kernels (no exact-fp32 mode)
H = W = 256
SC, SF = 64, 128
NEAR, FAR, FOV = 2.0 / 3.0, 5.0 / 3.0, 0.6911112
N_TRAIN = 4096


def make_ctx(lx, ld, precision="f16x3", alpha=0.05):
    kw = dict(n_pos_enc_xyz=lx, n_pos_enc_dir=ld, n_angles=2)
    ctx = N.Context(near=NEAR, far=FAR, precision=precision, leaky_relu_alpha=alpha, **kw)
    ctx.load_weights(0, N.glorot_blob(0, **kw))
    ctx.load_weights(1, N.glorot_blob(1, **kw))
    ctx.use_torch_stream()
    return ctx


def main():
    c2w = O.get_sphere_matrix(1.0, -30.0, 45.0, 0.0).astype(np.float32)
    render = {(lx, ld, p): make_ctx(lx, ld, p) for lx, ld in GEOMS for p in ("fp32", "f16x3", "f16")
              if lx <= 5 or p != "fp32"}
    train = {}
    g = torch.Generator(device="cuda").manual_seed(0)
    o = torch.zeros((N_TRAIN, 4), device="cuda"); o[:, 2] = 1.0; o[:, 3] = 1.0
    d = torch.randn((N_TRAIN, 4), device="cuda", generator=g) * 0.3; d[:, 2] = -1.0; d[:, 3] = 0.0
    tgt = torch.rand((N_TRAIN, 3), device="cuda", generator=g)
    for lx, ld in GEOMS:
        for policy in ("float32", "mixed_float16"):
            ctx = make_ctx(lx, ld)
            ctx.train_begin(5e-4, mixed_float16=policy == "mixed_float16")
            train[(lx, ld, policy)] = ctx

    def time_render(ctx, seed0):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(STEPS):
            ctx.render_image(c2w, FOV, H, W, H * W, SC, SF, seed=seed0 + i, device_out=True, rgb_only=True)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / STEPS

    def time_train(ctx, seed0):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(STEPS):
            ctx.train_step(o, d, tgt, SC, SF, seed=seed0 + i, want_metrics=False)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / STEPS

    for k, ctx in render.items():          # warm-up: code objects, arenas
        time_render(ctx, 0)
    for k, ctx in train.items():
        time_train(ctx, 0)
    rt = {k: [] for k in render}
    tt = {k: [] for k in train}
    for r in range(ROUNDS):
        for k, ctx in render.items():
            rt[k].append(time_render(ctx, 1000 * (r + 1)))
        for k, ctx in train.items():
            tt[k].append(time_train(ctx, 1000 * (r + 1)))
    out = {"what": "encoding geometry cost: render 256x256 64+128 (rays/s), train step 4096 rays 64+128 (ms)",
           "rounds": ROUNDS, "steps_per_measurement": STEPS, "device": torch.cuda.get_device_name(0),
           "render_rays_per_s": {}, "render_rate_vs_5_4": {}, "train_ms": {}, "train_time_vs_5_4": {}}
    for (lx, ld, p), v in rt.items():
        rate = H * W / float(np.median(v))
        out["render_rays_per_s"][f"Lx{lx}_Ld{ld}_{p}"] = round(rate)
    for (lx, ld, p), v in rt.items():
        base = out["render_rays_per_s"][f"Lx5_Ld4_{p}"]
        out["render_rate_vs_5_4"][f"Lx{lx}_Ld{ld}_{p}"] = round(out["render_rays_per_s"][f"Lx{lx}_Ld{ld}_{p}"] / base, 4)
    for (lx, ld, p), v in tt.items():
        out["train_ms"][f"Lx{lx}_Ld{ld}_{p}"] = round(float(np.median(v)) * 1e3, 3)
    for (lx, ld, p), v in tt.items():
        out["train_time_vs_5_4"][f"Lx{lx}_Ld{ld}_{p}"] = round(out["train_ms"][f"Lx{lx}_Ld{ld}_{p}"] /
                                                              out["train_ms"][f"Lx5_Ld4_{p}"], 4)
    for ctx in list(render.values()) + list(train.values()):
        ctx.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
