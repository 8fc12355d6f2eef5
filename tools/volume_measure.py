"""Measurements for the radiance volume (profiles/volume_measure.json), on one MI355X, shipped epoch-95
checkpoint, fine network, f16x3, device-resident arrays, times by a host clock around a device synchronise:
  bake      NeRF.bake_preview (camera mode, the test pose) at n = 128, 256, 512: median of three calls after one warm-up call
  frame     a 256 x 256 preview frame of the test pose through the n = 256 volume at 512 steps per ray, t_min 0 and 1/512, and the
            network frame at 64 + 128 samples under the same scene box, the three alternating inside each of ten rounds after
            two warm-up rounds; the march's gather rate at t_min = 0: (rays that hit the box) x 512 steps x 8 texels x 16 bytes
            over the frame time
  quality   at the fixture's resolution, for n = 64, 128, 256, 512 with 2 n steps and t_min = 1 / 512, a camera-mode bake and a
            constant-direction bake: PSNR of the preview against the network render (under the same scene box, without it, and on
            the pixels the preview leaves opaque) and against the held-out photograph, beside the network render's own PSNR
            against the photograph with and without the box

    python tools/volume_measure.py [OUT.json]        (default: volume_measure.json in the current directory)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))       # the repository: this file lives in tools/
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import nerf_and_dietnerf_amd as N  # noqa: E402

OUT = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else "volume_measure.json")
BOX = ((-0.6, -0.4, -1.3), (0.4, 0.8, -0.4))                              # around the golden scene's content
NET = {"hidden_layer_dim": 256, "last_hidden_layer_dim": 128, "leaky_relu_alpha": 0.05, "n_pos_enc_dim_xyz": 5,
       "n_pos_enc_view_dir": 4, "n_angles_for_model": 2}
T_MIN = 1.0 / 512.0


def clock(model, call):
    torch.cuda.synchronize()
    model.ctx.synchronize()
    t0 = time.perf_counter()
    out = call()
    model.ctx.synchronize()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stats(times):
    return {"median_ms": float(np.median(times)), "min_ms": float(min(times)), "max_ms": float(max(times)),
            "std_ms": float(np.std(times))}


def psnr(a, b):
    return float(-10.0 * np.log10(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


ck = np.load(os.path.join(ROOT, "tests", "golden", "alexander50_epoch095.npz"))
near, far, fov, c2w = float(ck["near"]), float(ck["far"]), float(ck["fov"]), ck["c2w_test"]
rc = {"n_render_samples_coarse": 64, "n_render_samples_fine": 128, "scene_box": [list(BOX[0]), list(BOX[1])]}
model = N.NeRF(NET, rc, near, far, precision="f16x3")
model.set_weights(ck["blob_coarse"], ck["blob_fine"])
res = {"what": "radiance volume: bake, preview frame and preview quality; shipped epoch-95 checkpoint, fine network, f16x3, "
               "device-resident arrays, one MI355X; host clock around a device synchronise",
       "command": "python tools/volume_measure.py", "box": BOX, "t_min": T_MIN}

# ---- bake ----
res["bake"] = {}
for n in (128, 256, 512):
    times = [clock(model, lambda: model.bake_preview(n, camera=c2w))[0] for _ in range(4)][1:]
    res["bake"][str(n)] = dict(stats(times), points=n ** 3, volume_bytes=16 * n ** 3,
                               points_per_s=n ** 3 / (float(np.median(times)) * 1e-3))
    print("bake", n, res["bake"][str(n)], flush=True)
    model._preview = None
    torch.cuda.empty_cache()

# ---- frame ----
H = W = 256
model.bake_preview(256, camera=c2w)
volume, lo, hi, _ = model._preview
calls = {
    "preview_t_min_0": lambda: model.render_preview(c2w, fov, H, W, n_steps=512, t_min=0.0),
    "preview_t_min_1_512": lambda: model.render_preview(c2w, fov, H, W, n_steps=512, t_min=T_MIN),
    "network_64_128": lambda: model.render_image(c2w, fov, H, W, seed=0, device_out=True, rgb_only=True),
}
times = {k: [] for k in calls}
for rnd in range(12):
    for k, call in calls.items():
        ms, _ = clock(model, call)
        if rnd >= 2:
            times[k].append(ms)
ones = torch.ones_like(volume[:3, :3, :3])
hits = int((model.ctx.render_volume_image(ones, lo, hi, c2w, fov, H, W, 1)[2] > 0).sum().item())
res["frame"] = {"height": H, "width": W, "n": 256, "n_steps": 512, "rounds": 10, "rays_that_hit_the_box": hits,
                **{k: stats(v) for k, v in times.items()}}
gather_bytes = hits * 512 * 8 * 16
res["frame"]["gather_bytes_t_min_0"] = gather_bytes
res["frame"]["gather_rate_TB_per_s_t_min_0"] = gather_bytes / (res["frame"]["preview_t_min_0"]["median_ms"] * 1e-3) / 1e12
res["frame"]["network_over_preview_t_min_1_512"] = (res["frame"]["network_64_128"]["median_ms"]
                                                     / res["frame"]["preview_t_min_1_512"]["median_ms"])
print("frame", res["frame"], flush=True)

# ---- quality ----
photo = ck["img_test"].astype(np.float64) / 255.0
h, w = photo.shape[:2]
net = model.render_image(c2w, fov, h, w, seed=0)[0].reshape(h, w, 3)
model.ctx.set_scene_box(None)                  # the network render the checkpoint's 27.8 dB was recorded with: no box
net_no_box = model.render_image(c2w, fov, h, w, seed=0)[0].reshape(h, w, 3)
model.ctx.set_scene_box(*BOX)
res["quality"] = {"height": h, "width": w, "network_vs_photograph_db": psnr(net, photo),
                  "network_without_box_vs_photograph_db": psnr(net_no_box, photo),
                  "recorded_network_vs_photograph_db": float(ck["recorded_psnr_test"]), "preview": {}}
for n in (64, 128, 256, 512):
    row = {}
    for mode, kw in (("camera", {"camera": c2w}), ("constant_direction", {})):
        model.bake_preview(n, **kw)
        rgb, _, opacity = model.render_preview(c2w, fov, h, w)
        rgb, opaque = rgb.cpu().numpy(), (opacity > 0.99).cpu().numpy()
        row[mode] = {"vs_network_db": psnr(rgb, net), "vs_photograph_db": psnr(rgb, photo),
                     "vs_network_without_box_db": psnr(rgb, net_no_box),
                     "mean_opacity": float(opacity.mean().item()), "pixels_with_opacity_above_0.99": int(opaque.sum()),
                     "vs_network_on_those_pixels_db": psnr(rgb[opaque], net[opaque]) if opaque.any() else None}
        model._preview = None
        torch.cuda.empty_cache()
    res["quality"]["preview"][str(n)] = row
    print("quality", n, row, flush=True)
model.ctx.close()

os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res, indent=1))
