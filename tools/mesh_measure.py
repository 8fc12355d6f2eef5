"""Measurements for mesh extraction (profiles/mesh_measure.json), on one MI355X: the three stages of
NeRF.extract_mesh at n = 256 on the shipped checkpoint's fine network in f16x3, device-resident arrays, the threshold the median
of the positive lattice values -- density_lattice, isosurface + fetch, mesh_colors -- each as the median of ten calls after two
warm-up calls, by a host clock around a device synchronise; the time the MLP kernels take inside density_lattice (stream events,
nerf_ctx_enable_timing) and the lattice's row rate; the isosurface at n = 512 on the same field resampled by repetition.

    python tools/mesh_measure.py [OUT.json]        (default: mesh_measure.json in the current directory)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))       # the repository: this file lives in tools/
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import nerf_and_dietnerf_amd as N  # noqa: E402

OUT = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else "mesh_measure.json")
BOX = ((-0.6, -0.4, -1.3), (0.4, 0.8, -0.4))                              # around the golden scene's content
WARMUP, CALLS = 2, 10


def timed(ctx, call):
    """Median and spread (ms) of CALLS calls after WARMUP, each ended by a device synchronise; and the last result."""
    times = []
    for i in range(WARMUP + CALLS):
        torch.cuda.synchronize()
        ctx.synchronize()
        t0 = time.perf_counter()
        out = call()
        ctx.synchronize()
        torch.cuda.synchronize()
        if i >= WARMUP:
            times.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": float(np.median(times)), "min_ms": float(min(times)), "max_ms": float(max(times))}, out


ck = np.load(os.path.join(ROOT, "tests", "golden", "alexander50_epoch095.npz"))
ctx = N.Context(near=float(ck["near"]), far=float(ck["far"]), precision="f16x3")
ctx.load_weights(0, ck["blob_coarse"])
ctx.load_weights(1, ck["blob_fine"])
ctx.set_scene_box(*BOX)
n = 256
res = {"what": "NeRF.extract_mesh stage by stage, shipped epoch-95 fine network, f16x3, device-resident arrays, one MI355X; "
               f"medians of {CALLS} calls after {WARMUP} warm-up calls, host clock around a device synchronise",
       "command": "python tools/mesh_measure.py", "n": n, "box": BOX}

res["density_lattice"], sigma = timed(ctx, lambda: ctx.density_lattice(1, n, device_out=True))
ctx.enable_timing(True)
ctx.read_timing()
ctx.density_lattice(1, n, device_out=True)
mlp_ms, launches, rows = ctx.read_timing()
ctx.enable_timing(False)
res["density_lattice"].update({"points": n ** 3, "mlp_kernel_ms": mlp_ms, "mlp_launches": launches, "mlp_rows": rows,
                               "rows_per_s_call": n ** 3 / (res["density_lattice"]["median_ms"] * 1e-3),
                               "rows_per_s_mlp_kernels": rows / (mlp_ms * 1e-3)})
positive = sigma[sigma > 0]
thr = float(positive.median())
res["sigma_threshold"] = thr
res["isosurface_and_fetch"], (v, t, nrm) = timed(ctx, lambda: ctx.isosurface(sigma, BOX[0], BOX[1], thr))
res["isosurface_and_fetch"].update({"vertices": int(v.shape[0]), "triangles": int(t.shape[0]), "volume_bytes": 4 * n ** 3})
res["mesh_colors"], rgb = timed(ctx, lambda: ctx.mesh_colors(1, v, nrm))
res["mesh_colors"]["rows_per_s_call"] = int(v.shape[0]) / (res["mesh_colors"]["median_ms"] * 1e-3)
res["isosurface_share_of_network_time"] = res["isosurface_and_fetch"]["median_ms"] / (
    res["density_lattice"]["median_ms"] + res["mesh_colors"]["median_ms"])
del v, t, nrm, rgb

big = sigma.repeat_interleave(2, 0).repeat_interleave(2, 1).repeat_interleave(2, 2).contiguous()      # 512^3, blocky
del sigma
res["isosurface_and_fetch_512"], (v, t, nrm) = timed(ctx, lambda: ctx.isosurface(big, BOX[0], BOX[1], thr))
res["isosurface_and_fetch_512"].update({"vertices": int(v.shape[0]), "triangles": int(t.shape[0]), "volume_bytes": 4 * 512 ** 3})
ctx.close()

os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res, indent=1))
