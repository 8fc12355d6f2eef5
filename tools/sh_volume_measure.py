"""Measurements for the SH radiance volume (profiles/sh_volume_measure.json), on one MI355X, shipped epoch-95
checkpoint, fine network, f16x3, device-resident arrays, times by a host clock around a device synchronise:
  bake      NeRF.bake_preview(n, sh_degree=L), default table, L = 0..3 at n = 128 and 256: median of three calls after one
            warm-up call
  frame     a 256 x 256 preview frame of the test pose through the n = 256 volume at 512 steps per ray, t_min = 0 and 1 / 512, for
            L = 0..3 and the degree-less march (camera bake), beside the network frame at 64 + 128 samples under the same box,
            all alternating inside each of ten rounds after two warm-up rounds; the march's gather rate: (rays that hit the box)
            x 512 steps x 8 texels x the texel's bytes over the frame time at t_min = 0
  mappings  the marched frames (SH and plain, t_min = 0 and 1 / 512) in fresh processes, alternating between two builds of this
            library that force one mapping of the march for every degree, -DNERF_SH_MARCH_LANES=8 (eight lanes per ray) and
            =1 (one lane per ray), two processes each; the two must give the same bits as each other and as the shipped
            choice, and a checksum of every frame says so
  parent_lib  the same frames in fresh processes alternating between a build of the parent commit's library and this tree's,
            three each: whether every frame has the same bits in all six, and per frame whether the median of this tree's
            process medians exceeds the parent's by more than the range of the parent's own three
  bench     bench.py --gpus 1 in fresh processes alternating between a checkout of the parent commit (built) and this tree,
            two each
  quality   at the fixture's resolution, n = 128 and 256 with 2 n steps and t_min = 1 / 512, at the golden test pose and at
            that pose carried 50 degrees of azimuth around the box: PSNR of the preview against the network render of the same
            pose, over the whole frame and over the pixels the preview leaves opaque, for a constant-direction bake, a camera
            bake made AT THE GOLDEN POSE, and SH degrees 0..3 with the default table

    python tools/sh_volume_measure.py [OUT.json] [--lanes1-lib LIB.so --lanes8-lib LIB.so] [--parent-lib LIB.so]
                                      [--parent-tree DIR] [--fresh-processes-only]
(default OUT: sh_volume_measure.json in the current directory; a section whose libraries or tree are not given is recorded as
"not measured"; --fresh-processes-only leaves out bake, frame and quality, the sections this process measures itself).  A
forced build: make -C nerf_and_dietnerf_amd/csrc EXTRA=-DNERF_SH_MARCH_LANES=1 OUT=<dir> BUILD=<dir>."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))       # the repository: this file lives in tools/
sys.path.insert(0, ROOT)

BOX = ((-0.6, -0.4, -1.3), (0.4, 0.8, -0.4))                              # around the golden scene's content
NET = {"hidden_layer_dim": 256, "last_hidden_layer_dim": 128, "leaky_relu_alpha": 0.05, "n_pos_enc_dim_xyz": 5,
       "n_pos_enc_view_dir": 4, "n_angles_for_model": 2}
T_MIN = 1.0 / 512.0
H = W = 256
DEGREES = (0, 1, 2, 3)


def stats(times):
    return {"median_ms": float(np.median(times)), "min_ms": float(min(times)), "max_ms": float(max(times)),
            "std_ms": float(np.std(times))}


def psnr(a, b):
    return float(-10.0 * np.log10(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


def orbit(c2w, centre, degrees):
    """The camera carried ``degrees`` of azimuth around ``centre`` about its own up axis, still looking at what it looked at."""
    c = np.asarray(c2w, np.float64).reshape(4, 4)
    k = c[:3, 1] / np.linalg.norm(c[:3, 1])
    kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    t = np.radians(degrees)
    rot = np.eye(3) + np.sin(t) * kx + (1 - np.cos(t)) * (kx @ kx)
    out = c.copy()
    out[:3, :3] = rot @ c[:3, :3]
    out[:3, 3] = np.asarray(centre) + rot @ (c[:3, 3] - np.asarray(centre))
    return out.astype(np.float32)


def make_model():
    import nerf_and_dietnerf_amd as N
    ck = np.load(os.path.join(ROOT, "tests", "golden", "alexander50_epoch095.npz"))
    rc = {"n_render_samples_coarse": 64, "n_render_samples_fine": 128, "scene_box": [list(BOX[0]), list(BOX[1])]}
    model = N.NeRF(NET, rc, float(ck["near"]), float(ck["far"]), precision="f16x3")
    model.set_weights(ck["blob_coarse"], ck["blob_fine"])
    return model, ck


def clock(model, call):
    import torch
    torch.cuda.synchronize()
    model.ctx.synchronize()
    t0 = time.perf_counter()
    out = call()
    model.ctx.synchronize()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def time_round_robin(model, calls, rounds=10, warmup=2):
    times = {k: [] for k in calls}
    for rnd in range(warmup + rounds):
        for k, call in calls.items():
            ms, _ = clock(model, call)
            if rnd >= warmup:
                times[k].append(ms)
    return {k: stats(v) for k, v in times.items()}


T_MINS = (("t_min_0", 0.0), ("t_min_1_512", T_MIN))


def sh_frames(model, ck, network):
    """The frame section: every SH degree's n = 256 volume resident, marched in turn beside the plain march (camera bake)
    and, with ``network``, the network frame -> (stats, checksums of every marched frame's rgb)."""
    c2w, fov = ck["c2w_test"], float(ck["fov"])
    ctx = model.ctx
    calls = {}
    for degree in DEGREES:
        model.bake_preview(256, sh_degree=degree)
        vol, lo, hi, _ = model._preview
        for name, t_min in T_MINS:
            calls[f"sh{degree}_{name}"] = (lambda v=vol, t=t_min: ctx.render_sh_volume_image(v, lo, hi, c2w, fov, H, W, 512, t))
    model.bake_preview(256, camera=c2w)
    plain, lo, hi, _ = model._preview
    for name, t_min in T_MINS:
        calls[f"plain_{name}"] = (lambda t=t_min: ctx.render_volume_image(plain, lo, hi, c2w, fov, H, W, 512, t))
    sums = {k: hashlib.sha256(call()[0].cpu().numpy().tobytes()).hexdigest()[:16] for k, call in calls.items()}
    if network:
        calls["network_64_128"] = lambda: model.render_image(c2w, fov, H, W, seed=0, device_out=True, rgb_only=True)
    return time_round_robin(model, calls), sums


def child_frames(out_path):
    model, ck = make_model()
    frames, sums = sh_frames(model, ck, network=False)
    model.ctx.close()
    with open(out_path, "w") as f:
        json.dump({"frames": frames, "checksums": sums}, f)


def run_child(lib, out_path):
    env = dict(os.environ)
    if lib:
        env["NERF_MI355_LIB"] = os.path.abspath(lib)
    subprocess.run([sys.executable, os.path.abspath(__file__), "--child-frames", out_path], check=True, env=env, timeout=600)
    with open(out_path) as f:
        return json.load(f)


def run_bench(tree):
    tree = os.path.abspath(tree)
    p = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"],
                       check=True, cwd=tree, timeout=600, stdout=subprocess.PIPE, text=True)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
    return json.loads(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default="sh_volume_measure.json")
    ap.add_argument("--lanes1-lib")
    ap.add_argument("--lanes8-lib")
    ap.add_argument("--parent-tree")
    ap.add_argument("--parent-lib")
    ap.add_argument("--fresh-processes-only", action="store_true")
    ap.add_argument("--child-frames")
    args = ap.parse_args()
    if args.child_frames:
        return child_frames(args.child_frames)
    out_path = os.path.abspath(args.out)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    sections = "" if args.fresh_processes_only else "bake, preview frame, preview quality, "
    res = {"what": f"SH radiance volume: {sections}the two march mappings, the parent commit's library against this one, bench.py "
                   "against the parent; shipped epoch-95 checkpoint, fine network, f16x3, device-resident arrays, one MI355X; "
                   "host clock around a device synchronise",
           "command": "python tools/sh_volume_measure.py" + (" --fresh-processes-only" if args.fresh_processes_only else ""),
           "box": BOX, "t_min": T_MIN}

    def save():
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)

    sums = None if args.fresh_processes_only else one_process_sections(res, save)
    fresh_process_sections(args, res, save, sums, out_path)
    print(json.dumps(res, indent=1))


def one_process_sections(res, save):
    """bake, frame and quality, in this process -> the checksums of the frame section."""
    import torch
    from nerf_and_dietnerf_amd import sh_quadrature, sh_texel_floats
    model, ck = make_model()
    c2w, fov = ck["c2w_test"], float(ck["fov"])
    # ---- bake ----
    res["bake"] = {}
    for n in (128, 256):
        for degree in DEGREES:
            times = [clock(model, lambda: model.bake_preview(n, sh_degree=degree))[0] for _ in range(4)][1:]
            d = len(sh_quadrature(degree)[0])
            res["bake"][f"n{n}_sh{degree}"] = dict(stats(times), vertices=n ** 3, directions=d, network_points=n ** 3 * d,
                                                   volume_bytes=4 * sh_texel_floats(degree) * n ** 3,
                                                   network_points_per_s=n ** 3 * d / (float(np.median(times)) * 1e-3))
            print("bake", n, degree, res["bake"][f"n{n}_sh{degree}"], flush=True)
            model._preview = None
            torch.cuda.empty_cache()
    save()
    # ---- frame ----
    frames, sums = sh_frames(model, ck, network=True)
    ones = torch.ones((3, 3, 3, 4), device="cuda")
    hits = int((model.ctx.render_volume_image(ones, BOX[0], BOX[1], c2w, fov, H, W, 1)[2] > 0).sum().item())
    res["frame"] = {"height": H, "width": W, "n": 256, "n_steps": 512, "rounds": 10, "rays_that_hit_the_box": hits,
                    "mapping": "as shipped: one lane per ray at degrees 0 and 1, eight at 2 and 3", **frames}
    for degree in DEGREES:
        gathered = hits * 512 * 8 * 4 * sh_texel_floats(degree)
        res["frame"][f"sh{degree}_gather_TB_per_s_t_min_0"] = gathered / (frames[f"sh{degree}_t_min_0"]["median_ms"] * 1e-3) / 1e12
    print("frame", res["frame"], flush=True)
    save()
    # ---- quality ----
    h, w = ck["img_test"].shape[:2]
    centre = 0.5 * (np.array(BOX[0]) + np.array(BOX[1]))
    poses = {"golden_pose": np.asarray(c2w, np.float32), "azimuth_50_degrees_away": orbit(c2w, centre, 50.0)}
    nets = {k: model.render_image(p, fov, h, w, seed=0)[0].reshape(h, w, 3) for k, p in poses.items()}
    bakes = [("constant_direction", {}), ("camera_at_golden_pose", {"camera": poses["golden_pose"]})] + \
            [(f"sh{degree}", {"sh_degree": degree}) for degree in DEGREES]
    res["quality"] = {"height": h, "width": w, "opaque_means": "opacity > 0.99", "preview": {}}
    for n in (128, 256):
        for label, kw in bakes:
            model.bake_preview(n, **kw)
            row = {}
            for pose, p in poses.items():
                rgb, _, opacity = model.render_preview(p, fov, h, w)
                rgb, opaque = rgb.cpu().numpy(), (opacity > 0.99).cpu().numpy()
                row[pose] = {"vs_network_db": psnr(rgb, nets[pose]), "opaque_pixels": int(opaque.sum()),
                             "vs_network_on_opaque_pixels_db": psnr(rgb[opaque], nets[pose][opaque]) if opaque.any() else None}
            res["quality"]["preview"][f"n{n}_{label}"] = row
            print("quality", n, label, row, flush=True)
            model._preview = None
            torch.cuda.empty_cache()
    model.ctx.close()
    del model
    torch.cuda.empty_cache()
    save()
    return sums


def alternate(libs, rounds, sums, out_path):
    """Fresh child-frame processes, the libraries ``libs`` (name -> path, None: this tree's) in turn, ``rounds`` times ->
    (whether every frame's checksum is the same in all of them and in ``sums`` if given, name -> frame -> each process's
    median_ms)."""
    runs = {name: [] for name in libs}
    for rnd in range(rounds):
        for name, lib in libs.items():
            runs[name].append(run_child(lib, out_path + f".child_{name}_{rnd}.json"))
            os.remove(out_path + f".child_{name}_{rnd}.json")
            print(name, rnd, runs[name][-1]["frames"], flush=True)
    all_sums = [r["checksums"] for v in runs.values() for r in v] + ([sums] if sums else [])
    return all(s == all_sums[0] for s in all_sums), \
        {name: {k: [r["frames"][k]["median_ms"] for r in v] for k in v[0]["frames"]} for name, v in runs.items()}


def fresh_process_sections(args, res, save, sums, out_path):
    # ---- the two mappings, alternating processes ----
    if args.lanes1_lib and args.lanes8_lib and os.path.exists(args.lanes1_lib) and os.path.exists(args.lanes8_lib):
        same, medians = alternate({"eight_lanes_per_ray": args.lanes8_lib, "one_lane_per_ray": args.lanes1_lib}, 2, sums, out_path)
        res["mappings"] = {"what": "fresh processes, A B A B; median_ms of each process's ten rounds",
                           "same_bits_in_every_process_and_mapping": same, **medians}
    else:
        res["mappings"] = "not measured (no --lanes1-lib and --lanes8-lib)"
    save()
    # ---- the parent commit's library against this tree's, alternating processes ----
    if args.parent_lib and os.path.exists(args.parent_lib):
        same, medians = alternate({"parent": args.parent_lib, "this": None}, 3, sums, out_path)
        # a frame is no slower when the median of this tree's process medians exceeds the parent's by no more than the range
        # (max - min) of the parent's own process medians: the run-to-run spread of the same call
        verdict = {k: {"parent_median_ms": float(np.median(p)), "this_median_ms": float(np.median(medians["this"][k])),
                       "parent_range_ms": max(p) - min(p),
                       "no_slower": bool(np.median(medians["this"][k]) - np.median(p) <= max(p) - min(p))}
                   for k, p in medians["parent"].items()}
        res["parent_lib"] = {"what": "fresh processes, parent / this three times; median_ms of each process's ten rounds",
                             "same_bits_in_every_process": same, **medians, "verdict": verdict}
    else:
        res["parent_lib"] = "not measured (no --parent-lib)"
    save()
    # ---- bench.py against the parent commit ----
    if args.parent_tree and os.path.exists(os.path.join(args.parent_tree, "bench.py")):
        runs = {"this": [], "parent": []}
        for rnd in range(2):
            for name, tree in (("parent", args.parent_tree), ("this", ROOT)):
                runs[name].append(run_bench(tree))
                print("bench", name, rnd, runs[name][-1], flush=True)
        res["bench"] = {"what": "bench.py --gpus 1 --steps 20 --warmup 5, fresh processes, parent / this / parent / this", **runs}
    else:
        res["bench"] = "not measured (no --parent-tree)"
    save()


if __name__ == "__main__":
    main()
