"""Measurements for the rgb-skipping fine kernel of the f16x3 mode (profiles/rgb_skip_ab.json), on one MI355X:

1. the share of 128-row groups of the fine launch that the kernel skips, counted on the host from a six-output run (alpha == 0
   throughout a group; the six-output run itself never skips): the benchmark's 256^2 x (64+128) frame with its Glorot blobs,
   and the shipped checkpoint's held-out view at the same size;
2. the MLP launches of an rgb_only frame by stream events (read_timing): coarse (sigma-only) and fine (rgb-skipping) launch;
3. with a diagnostics build (make EXTRA=-DNERF_STAMPS, NERF_MI355_LIB pointing at it): cycles per 32-row tile by phase of wave 0
   of workgroup 0 for a launch in which every group is skipped (sigma bias -50) and one in which none is (+1.5), next to the
   full kernel's phases on the same rows.

    python tools/rgb_skip_measure.py [OUT.json]        (default: rgb_skip_measure.json in the current directory)"""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))       # the repository: this file lives in tools/
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import nerf_and_dietnerf_amd as N  # noqa: E402

OUT = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else "rgb_skip_measure.json")
H = W = 256
SC, SF = bench.SC, bench.SF
res = {}


def save():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1)


def skipped_share(ctx, c2w, fov, seed):
    """six outputs of the frame in 4096-ray slabs -> (share of all-empty 128-row groups of the fine launch, share of samples
    with alpha == 0); a slab of 4096 rays x 192 samples is a whole number of groups, as the one-launch frame's rows are"""
    groups = empty = zero = total = 0
    for b in range(0, H * W, 4096):
        alpha = np.asarray(ctx.render_image(c2w, fov, H, W, 0, SC, SF, seed=seed, ray_begin=b, ray_count=4096)[3], np.float32)
        g = (alpha.reshape(-1, 128) == 0)
        groups += g.shape[0]
        empty += int(g.all(axis=1).sum())
        zero += int(g.sum())
        total += g.size
    return empty / groups, zero / total


def launch_times(ctx, c2w, fov, frames=10):
    for i in range(3):
        ctx.render_image(c2w, fov, H, W, 1 << 18, SC, SF, seed=i, device_out=True, rgb_only=True)
    ctx.synchronize()
    ctx.enable_timing(True)
    for i in range(frames):
        ctx.render_image(c2w, fov, H, W, 1 << 18, SC, SF, seed=10 + i, device_out=True, rgb_only=True)
    ms, launches, rows = ctx.read_timing()
    ctx.enable_timing(False)
    return {"mlp_ms_per_frame": ms / frames, "mlp_launches_per_frame": launches / frames, "mlp_rows_per_frame": rows / frames}


def frame_entry(name, blob_c, blob_f, near, far, c2w, fov):
    ctx = N.Context(near=near, far=far, precision="f16x3")
    ctx.load_weights(0, blob_c)
    ctx.load_weights(1, blob_f)
    entry = {"frame": f"{H}x{W} x ({SC}+{SF}), f16x3"}
    for seed in (2, 7):
        g, z = skipped_share(ctx, c2w, fov, seed)
        entry[f"seed_{seed}"] = {"groups_all_empty": g, "samples_with_alpha_0": z}
    entry["rgb_only_frame"] = launch_times(ctx, c2w, fov)
    ctx.close()
    res[name] = entry
    save()
    print(name, json.dumps(entry), flush=True)


C2W = bench.sphere_matrix(1.0, -30.0, 45.0, 0.0)
frame_entry("bench_frame_glorot", N.glorot_blob(0), N.glorot_blob(1), bench.NEAR, bench.FAR, C2W, bench.FOV)
g = np.load(os.path.join(ROOT, "tests", "golden", "alexander50_epoch095.npz"))
frame_entry("shipped_checkpoint_test_view", g["blob_coarse"], g["blob_fine"], float(g["near"]), float(g["far"]), g["c2w_test"],
            float(g["fov"]))

# ---- 3. the phase table (diagnostics build only) ----------------------------------------------------------------------------
lib = N._lib.load()
if hasattr(lib, "nerf_debug_read_stamps_h"):
    NAMES = ["prologue", "L0(PE)", "HID x6", "L4(SKIP)", "L8", "heads", "tiles", "vote", "skip: store + fast-forward", "skipped tiles"]

    def stamps():
        out = (ctypes.c_ulonglong * 16)()
        lib.nerf_debug_read_stamps_h(out)
        v = list(out)[:10]
        nt = max(v[6], 1)
        t = {n: (x if n in ("tiles", "skipped tiles") else round(x / nt, 1)) for n, x in zip(NAMES, v)}
        t["total_per_tile"] = round((sum(v[:6]) + v[7] + v[8]) / nt, 1)
        return t

    rng = np.random.default_rng(0)
    n, s = 256 * 64 * 128 // 64, 64                  # 64 tiles per workgroup of a 256-CU grid, as tools/stamps.py
    o = np.zeros((n, 4), np.float32)
    o[:, :3] = rng.uniform(-0.3, 0.3, (n, 3))
    o[:, 2] += 1.5
    d = np.zeros((n, 4), np.float32)
    d[:, :3] = rng.uniform(-0.4, 0.4, (n, 3))
    d[:, 2] = -1.0
    z = np.sort(rng.uniform(bench.NEAR, bench.FAR, (n, s)), axis=1).astype(np.float32)
    rgb = np.empty((n, 3), np.float32)
    rs = np.empty((n, s, 3), np.float32)
    table = {}
    for bias, label in ((-50.0, "every_group_skipped"), (1.5, "no_group_skipped")):
        blob = N.glorot_blob(1)
        blob[-1] = bias
        ctx = N.Context(near=bench.NEAR, far=bench.FAR, precision="f16x3")
        ctx.load_weights(0, blob)
        for want_samples in (False, True):
            outs = N._lib.NerfOutputs()
            outs.rgb = rgb.ctypes.data
            if want_samples:
                outs.rgb_samples = rs.ctypes.data
            # one launch: the context's first, so the per-launch gate (nerf_ctx.h: RgbSkipGate) knows nothing yet and the
            # rgb-skipping kernel runs also where nothing skips
            N._lib.check(lib.nerf_render_rays(ctx.h, 0, o.ctypes.data, d.ctypes.data, z.ctypes.data, n, s, ctypes.byref(outs),
                                              N._lib.NERF_MEM_HOST))
            table[label + (": full kernel" if want_samples else ": rgb-skipping kernel")] = stamps()
        ctx.close()
    res["stamps_cycles_per_tile"] = table
    save()
    print(json.dumps(table, indent=1), flush=True)
print("done", flush=True)
