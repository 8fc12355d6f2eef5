"""Measurements for sample culling under an occupancy grid (profiles/culling_measure.json), on one MI355X:

1. the benchmark's 256^2 x (64+128) frame (f16x3, Glorot weights) under tools/occupancy_measure.py's synthetic 128^3 grid (two
   balls plus 2 % scattered cells, 5.6 % full) in the box [-0.4, 0.4]^3: frame time with culling off and on, alternating inside
   each of twelve rounds of ten frames; the kept share; the MLP kernels' time per row on against off (read_timing); the culled
   passes' own stages by stream events (read_culling_timing);
2. the same frame under a FULL grid: every sample is kept, so on - off is the feature's pure overhead;
3. the shipped checkpoint's held-out view: fine PSNR against the golden image at 64+128 and 32+64 samples and rays/s on a
   256^2 frame of that pose, grid on, culling off and on.

    python tools/culling_measure.py [OUT.json]        (default: culling_measure.json in the current directory)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))       # the repository: this file lives in tools/
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import bench  # noqa: E402
import nerf_and_dietnerf_amd as N  # noqa: E402
import occupancy_ref as G  # noqa: E402

OUT = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else "culling_measure.json")
NET = {"hidden_layer_dim": 256, "last_hidden_layer_dim": 128, "leaky_relu_alpha": 0.05, "n_pos_enc_dim_xyz": 5,
       "n_pos_enc_view_dir": 4, "n_angles_for_model": 2, "n_rays_in_batch_train": 4096, "n_rays_in_batch_render": 4096}
res = {}


def save():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1)


def timed_frames(ctx, c2w, fov, h, w, sc, sf, frames, seed0):
    torch.cuda.synchronize()
    ctx.synchronize()
    t0 = time.perf_counter()
    for i in range(frames):
        ctx.render_image(c2w, fov, h, w, 1 << 18, sc, sf, seed=seed0 + i, device_out=True, rgb_only=True)
    ctx.synchronize()
    return (time.perf_counter() - t0) / frames


def stats(a):
    a = np.asarray(a, np.float64)
    return {"ms_per_frame_mean": float(a.mean()), "std": float(a.std(ddof=1)), "min": float(a.min()), "max": float(a.max()),
            "per_round_ms": a.round(4).tolist()}


def off_on(ctx, c2w, fov, h, w, sc, sf, rounds=12, frames=10):
    """Frame time with culling off and on, alternating inside every round; then one timed pass of each for the kernels."""
    for cull in (False, True):                                  # warm every shape and buffer
        ctx.set_sample_culling(cull)
        timed_frames(ctx, c2w, fov, h, w, sc, sf, 3, 0)
    per = {False: [], True: []}
    ctx.read_culling()
    for r in range(rounds):
        for cull in (False, True):
            ctx.set_sample_culling(cull)
            per[cull].append(timed_frames(ctx, c2w, fov, h, w, sc, sf, frames, 100 * r) * 1e3)
    samples, kept = ctx.read_culling()
    out = {"off": stats(per[False]), "on": stats(per[True]), "samples": samples, "kept": kept, "kept_share": kept / max(samples, 1)}
    diff = np.array(per[True]) - np.array(per[False])
    out["on_minus_off_ms"] = {"mean": float(diff.mean()), "std_of_round_differences": float(diff.std(ddof=1)),
                              "stderr": float(diff.std(ddof=1) / np.sqrt(len(diff)))}
    out["rays_per_s"] = {"off": float(h * w / (np.mean(per[False]) * 1e-3)), "on": float(h * w / (np.mean(per[True]) * 1e-3))}
    # the kernels by stream events: a pass of its own, so that the events do not sit in the frame times above
    for cull in (False, True):
        ctx.set_sample_culling(cull)
        ctx.enable_timing(True)
        timed_frames(ctx, c2w, fov, h, w, sc, sf, frames, 7)
        stages, passes = ctx.read_culling_timing()                # first: read_timing clears the stage events too
        ms, launches, rows = ctx.read_timing()
        ctx.enable_timing(False)
        entry = {"mlp_ms_per_frame": ms / frames, "mlp_launches_per_frame": launches / frames, "mlp_rows_per_frame": rows / frames,
                 "mlp_ns_per_row": ms * 1e6 / max(rows, 1)}
        if cull:
            entry["stages_ms_per_frame"] = dict(zip(("verdict_and_scan", "host_read_of_the_row_count", "gather", "expand"),
                                                    (s / frames for s in stages)))
            entry["culled_passes_per_frame"] = passes / frames
        out["kernels_on" if cull else "kernels_off"] = entry
    ctx.read_culling()
    ctx.set_sample_culling(False)
    return out


# ---- 1, 2. the benchmark's frame under the synthetic grid and under a full grid -------------------------------------------------
H = W = 256
SC, SF = bench.SC, bench.SF
model = N.NeRF(NET, {"n_render_samples_coarse": SC, "n_render_samples_fine": SF}, bench.NEAR, bench.FAR, precision="f16x3")
model.set_weights(N.glorot_blob(0), N.glorot_blob(1))
ctx = model.ctx
c2w = bench.sphere_matrix(1.0, -30.0, 45.0, 0.0)
LO, HI = (-0.4, -0.4, -0.4), (0.4, 0.4, 0.4)
grid128 = G.two_balls(128, np.array(LO, np.float32) * 2.5, np.array(HI, np.float32) * 2.5) | \
    (np.random.default_rng(1).random((128, 128, 128)) < 0.02)
ctx.set_scene_box(LO, HI)
for name, grid in (("synthetic", grid128), ("full_grid", np.ones((128, 128, 128), bool))):
    ctx.set_occupancy_grid(grid)
    entry = {"frame": f"{H}x{W} x ({SC}+{SF}), f16x3, Glorot weights, box {LO}..{HI}", "grid_fill": float(grid.mean())}
    entry.update(off_on(ctx, c2w, bench.FOV, H, W, SC, SF))
    res[name] = entry
    save()
    print(name, json.dumps({k: v for k, v in entry.items()}, indent=1), flush=True)
res["synthetic"]["grid"] = "two_balls(128) of tests/occupancy_ref.py | (default_rng(1).random((128,)*3) < 0.02), as tools/occupancy_measure.py"
ctx.close()

# ---- 3. the shipped checkpoint, the held-out view -------------------------------------------------------------------------------
g = np.load(os.path.join(ROOT, "tests", "golden", "alexander50_epoch095.npz"))
near, far, fov = float(g["near"]), float(g["far"]), float(g["fov"])
img = g["img_test"].astype(np.float32) / 255.0
c2w = g["c2w_test"]


def psnr(a, b):
    return float(-10 * np.log10(np.mean((a - b) ** 2)))


BOX = ((-1.5, -1.5, -2.2), (1.5, 1.5, 0.5))
res["quality"] = {"view": "held-out golden view (c2w_test), 50 x 50, f16x3, fine PSNR against the golden image, seeds 1-3; rays/s on "
                          "a 256 x 256 frame of the same pose; grid baked from the fine network, threshold 5, 2 points per cell, "
                          "dilate 1", "box": BOX, "rows": []}
m = N.NeRF(NET, {"n_render_samples_coarse": 64, "n_render_samples_fine": 128}, near, far, precision="f16x3")
m.set_weights(g["blob_coarse"], g["blob_fine"])
cx = m.ctx
cx.set_scene_box(*BOX)
for resolution in (128, 64):
    count = cx.bake_occupancy_grid(1, resolution, 5.0, 2, 1)
    for sc, sf in ((64, 128), (32, 64)):
        for cull in (False, True):
            cx.set_sample_culling(cull)
            cx.read_culling()
            ps = [psnr(cx.render_image(c2w, fov, 50, 50, 0, sc, sf, seed=s)[0], img) for s in (1, 2, 3)]
            samples, kept = cx.read_culling()
            timed_frames(cx, c2w, fov, 256, 256, sc, sf, 3, 0)
            t = [timed_frames(cx, c2w, fov, 256, 256, sc, sf, 10, 10 * k) for k in range(5)]
            res["quality"]["rows"].append({"resolution": resolution, "occupied_share": count / resolution ** 3, "samples": f"{sc}+{sf}",
                                           "culling": "on" if cull else "off", "psnr_seeds_1_2_3": ps, "psnr_mean": float(np.mean(ps)),
                                           "kept_share_50x50": kept / samples if samples else None,
                                           "rays_per_s_256x256": float(65536 / np.mean(t)),
                                           "ms_per_frame_rounds": (np.array(t) * 1e3).round(3).tolist()})
            print(json.dumps(res["quality"]["rows"][-1]), flush=True)
    save()
cx.close()
print("done", flush=True)
