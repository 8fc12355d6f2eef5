"""Measurements for the occupancy grid (profiles/occupancy_measure.json), on one MI355X:

1. cost of the pre-pass on the benchmark's 256^2 x (64+128) frame (f16x3, Glorot weights): no box / box / box + an R = 128 grid
   / an R = 64 grid, alternating inside each of twelve rounds of ten frames, and the depth launches alone by stream events.  The
   grid is synthetic, since a Glorot network has no density to bake: tests/occupancy_ref.py's two balls on 128^3 cells plus 2 %
   scattered cells (numpy seed 1), 5.6 % full; the R = 64 grid is every second cell of it;
2. what the grid buys: fine PSNR against the golden image of the shipped checkpoint's held-out view at 64+128 and 32+64 samples,
   grid off and on (baked from the fine network), for two boxes, and rays/s on a 256^2 frame of that pose.

    python tools/occupancy_measure.py [OUT.json]        (default: occupancy_measure.json in the current directory)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))       # the repository: this file lives in tools/
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import nerf_and_dietnerf_amd as N  # noqa: E402
import occupancy_ref as G  # noqa: E402

OUT = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else "occupancy_measure.json")
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


# ---- 1. the pre-pass on the benchmark's frame -------------------------------------------------------------------------------
import bench  # noqa: E402

H = W = 256
SC, SF = bench.SC, bench.SF
model = N.NeRF(NET, {"n_render_samples_coarse": SC, "n_render_samples_fine": SF}, bench.NEAR, bench.FAR, precision="f16x3")
model.set_weights(N.glorot_blob(0), N.glorot_blob(1))
ctx = model.ctx
c2w = bench.sphere_matrix(1.0, -30.0, 45.0, 0.0)
LO, HI = (-0.4, -0.4, -0.4), (0.4, 0.4, 0.4)
grid128 = G.two_balls(128, np.array(LO, np.float32) * 2.5, np.array(HI, np.float32) * 2.5) | \
    (np.random.default_rng(1).random((128, 128, 128)) < 0.02)
grid64 = grid128[::2, ::2, ::2].copy()


def arm(mode):
    ctx.set_scene_box(None)
    if mode != "plain":
        ctx.set_scene_box(LO, HI)
    if mode == "grid128":
        ctx.set_occupancy_grid(grid128)
    if mode == "grid64":
        ctx.set_occupancy_grid(grid64)


modes = ["plain", "box", "grid128", "grid64"]
for m in modes:                                      # warm every shape and buffer
    arm(m)
    timed_frames(ctx, c2w, bench.FOV, H, W, SC, SF, 3, 0)
arm("grid128")
dirs = ctx.get_rays_directions(H, W, bench.FOV, c2w).reshape(-1, 4)
orig = np.tile(np.asarray(c2w, np.float32)[:, 3], (H * W, 1))
_, state = ctx.ray_occupancy_bounds(orig, dirs)
res["prepass"] = {"frame": f"{H}x{W} x ({SC}+{SF}), f16x3, Glorot weights, box {LO}..{HI}",
                  "states_grid128": np.bincount(state, minlength=3).tolist(), "grid128_fill": float(grid128.mean()),
                  "grid": "two_balls(128) of tests/occupancy_ref.py | (default_rng(1).random((128,)*3) < 0.02); R = 64: every second cell"}
ROUNDS, FRAMES = 12, 10
per = {m: [] for m in modes}
for r in range(ROUNDS):                              # alternate the modes within every round
    for m in modes:
        arm(m)
        per[m].append(timed_frames(ctx, c2w, bench.FOV, H, W, SC, SF, FRAMES, 100 * r) * 1e3)
for m in modes:
    a = np.array(per[m])
    res["prepass"][m] = {"ms_per_frame_mean": float(a.mean()), "std": float(a.std(ddof=1)), "min": float(a.min()),
                         "max": float(a.max()), "rays_per_s": float(H * W / (a.mean() * 1e-3)), "per_round_ms": a.round(4).tolist()}
for m in ("grid128", "grid64"):
    diff = np.array(per[m]) - np.array(per["box"])
    res["prepass"][m + "_minus_box_ms"] = {"mean": float(diff.mean()), "std_of_round_differences": float(diff.std(ddof=1)),
                                           "stderr": float(diff.std(ddof=1) / np.sqrt(len(diff)))}
diff = np.array(per["box"]) - np.array(per["plain"])
res["prepass"]["box_minus_plain_ms"] = {"mean": float(diff.mean()), "stderr": float(diff.std(ddof=1) / np.sqrt(len(diff)))}
# the kernels alone, by stream events
o_t, d_t = torch.as_tensor(orig).cuda(), torch.as_tensor(dirs).cuda()
arm("grid128")
for name, call in (("ray_grid_bounds_kernel_R128", lambda: ctx.ray_occupancy_bounds(o_t, d_t)),
                   ("depths_with_grid_R128", lambda: ctx.get_z_values_for_rays(o_t, d_t, SC, seed=1))):
    ctx.use_torch_stream()
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(50):
        call()
    e1.record()
    torch.cuda.synchronize()
    res["prepass"][name + "_ms_per_call_incl_output_alloc"] = e0.elapsed_time(e1) / 50
arm("box")
call = lambda: ctx.get_z_values_for_rays(o_t, d_t, SC, seed=1)
for _ in range(3):
    call()
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(50):
    call()
e1.record()
torch.cuda.synchronize()
res["prepass"]["depths_with_box_only_ms_per_call_incl_output_alloc"] = e0.elapsed_time(e1) / 50
save()
print(json.dumps({k: v for k, v in res["prepass"].items() if k != "rounds"}, indent=1), flush=True)
ctx.close()

# ---- 2. what it buys: the shipped checkpoint, the held-out view ---------------------------------------------------------------
g = np.load(os.path.join(ROOT, "tests", "golden", "alexander50_epoch095.npz"))
near, far, fov = float(g["near"]), float(g["far"]), float(g["fov"])
img = g["img_test"].astype(np.float32) / 255.0
c2w = g["c2w_test"]


def psnr(a, b):
    return float(-10 * np.log10(np.mean((a - b) ** 2)))


res["quality"] = {"view": "held-out golden view (c2w_test), 50 x 50, f16x3, fine PSNR against the golden image; rays/s on a "
                          "256 x 256 frame of the same pose", "recorded_psnr_test": float(g["recorded_psnr_test"]), "boxes": {}}
BOXES = {"tight": ((-0.6, -0.4, -1.3), (0.4, 0.8, -0.4)), "wide": ((-1.5, -1.5, -2.2), (1.5, 1.5, 0.5))}
BAKE = dict(resolution=128, sigma_threshold=5.0, samples_per_cell=2, dilate=1)
for bname, (lo, hi) in BOXES.items():
    m = N.NeRF(NET, {"n_render_samples_coarse": 64, "n_render_samples_fine": 128}, near, far, precision="f16x3")
    m.set_weights(g["blob_coarse"], g["blob_fine"])
    cx = m.ctx
    entry = {"box": [lo, hi], "bake": BAKE, "rows": []}
    # no box at all, for orientation
    for sc, sf in ((64, 128), (32, 64)):
        ps = [psnr(cx.render_image(c2w, fov, 50, 50, 0, sc, sf, seed=s)[0], img) for s in (1, 2, 3)]
        entry["rows"].append({"samples": f"{sc}+{sf}", "box": "off", "grid": "off", "psnr_seeds_1_2_3": ps, "psnr_mean": float(np.mean(ps))})
    cx.set_scene_box(lo, hi)
    t0 = time.perf_counter()
    count = cx.bake_occupancy_grid(1, BAKE["resolution"], BAKE["sigma_threshold"], BAKE["samples_per_cell"], BAKE["dilate"])
    entry["bake_seconds_first_call"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    cx.bake_occupancy_grid(1, BAKE["resolution"], BAKE["sigma_threshold"], BAKE["samples_per_cell"], BAKE["dilate"])
    entry["bake_seconds_second_call"] = time.perf_counter() - t0
    grid = cx.occupancy_grid()
    entry["occupied_cells"], entry["occupied_share"] = count, count / BAKE["resolution"] ** 3
    d50 = cx.get_rays_directions(50, 50, fov, c2w).reshape(-1, 4)
    o50 = np.tile(np.asarray(c2w, np.float32)[:, 3], (2500, 1))
    bounds, state = cx.ray_occupancy_bounds(o50, d50)
    bb, _ = cx.ray_box_bounds(o50, d50)
    entry["states_50x50"] = np.bincount(state, minlength=3).tolist()
    entry["mean_interval_grid_over_box"] = float(np.mean((bounds[:, 1] - bounds[:, 0]) / (bb[:, 1] - bb[:, 0])))
    for sc, sf in ((64, 128), (32, 64)):
        for on in (False, True):
            cx.set_occupancy_grid(grid if on else None)
            ps = [psnr(cx.render_image(c2w, fov, 50, 50, 0, sc, sf, seed=s)[0], img) for s in (1, 2, 3)]
            timed_frames(cx, c2w, fov, 256, 256, sc, sf, 3, 0)
            t = [timed_frames(cx, c2w, fov, 256, 256, sc, sf, 10, 10 * k) for k in range(5)]
            entry["rows"].append({"samples": f"{sc}+{sf}", "box": "on", "grid": "on" if on else "off", "psnr_seeds_1_2_3": ps,
                                  "psnr_mean": float(np.mean(ps)), "rays_per_s_256x256": float(65536 / np.mean(t)),
                                  "ms_per_frame_rounds": (np.array(t) * 1e3).round(3).tolist()})
    res["quality"]["boxes"][bname] = entry
    save()
    print(json.dumps(entry, indent=1), flush=True)
    cx.close()
print("done", flush=True)
