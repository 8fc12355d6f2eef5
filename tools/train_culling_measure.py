"""Measurements for sample culling in the trainer (nerf_ctx_set_train_sample_culling; DESIGN.md 1.2,
profiles/train_culling_measure.json), on one MI355X: the training step bench.py times -- 4096 rays x (64+128), both policies,
train_step(want_metrics=False) enqueued back to back, one synchronise at the end -- in four settings:

1. flag off, no box: bench.py's own figure.  With --parent-root DIR (a checkout of the parent commit, built) the same loop runs on
   the parent's library too, in processes of their own that alternate with this build's, so that the flag-off path can be held to
   the parent's within the run-to-run spread of the rounds;
2. flag on under a FULL 128^3 grid: every sample kept, so on - off is the feature's pure overhead (verdict, scan, two host reads
   of a row count, gather, expand, the gather of dL/d(raw));
3. flag on under tools/culling_measure.py's synthetic 128^3 grid (two balls plus 2 % scattered cells) in the box [-0.4, 0.4]^3;
4. flag on under the grid baked from the shipped checkpoint (box [-1.5, 1.5]^2 x [-2.2, 0.5], R = 64, threshold 5, 2 points per
   cell, dilate 1: tests/test_gpu_culling.py::test_quality_on_the_shipped_checkpoint), on the rays of its two golden cameras.
Settings 2-4 alternate flag off and on inside every round, under the same grid (the grid narrows the depths either way), and
record the kept share.

    python tools/train_culling_measure.py [OUT.json] [--parent-root DIR]"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))       # the repository: this file lives in tools/
N_RAYS, ROUNDS, STEPS = 4096, 10, 20
POLICIES = ("float32", "mixed_float16")


def stats(a):
    a = np.asarray(a, np.float64)
    return {"ms_per_step_mean": float(a.mean()), "std_over_rounds": float(a.std(ddof=1)), "min": float(a.min()),
            "max": float(a.max()), "per_round_ms": a.round(4).tolist()}


def bench_batch(torch):
    """bench.py's training batch."""
    gen = torch.Generator(device="cuda").manual_seed(0)
    o = torch.zeros((N_RAYS, 4), device="cuda"); o[:, 2] = 1.0; o[:, 3] = 1.0
    d = torch.randn((N_RAYS, 4), device="cuda", generator=gen) * 0.3; d[:, 2] = -1.0; d[:, 3] = 0.0
    return o, d, torch.rand((N_RAYS, 3), device="cuda", generator=gen)


def timed_steps(ctx, torch, batch, sc, sf, steps, seed0):
    torch.cuda.synchronize()
    ctx.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        ctx.train_step(*batch, sc, sf, seed=seed0 + i, want_metrics=False)
    ctx.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def worker(root):
    """Setting 1 on the package under `root`: per policy, ROUNDS rounds of STEPS steps -> one JSON line."""
    sys.path.insert(0, root)
    import torch
    import bench
    import nerf_and_dietnerf_amd as N
    assert os.path.realpath(os.path.dirname(N.__file__)).startswith(os.path.realpath(root)), N.__file__
    batch = bench_batch(torch)
    out = {}
    for policy in POLICIES:
        ctx = N.Context(near=bench.NEAR, far=bench.FAR, precision="f16x3")
        ctx.load_weights(0, N.glorot_blob(0)); ctx.load_weights(1, N.glorot_blob(1))
        ctx.train_begin(5e-4, mixed_float16=policy == "mixed_float16")
        timed_steps(ctx, torch, batch, bench.SC, bench.SF, 5, 0)
        out[policy] = [timed_steps(ctx, torch, batch, bench.SC, bench.SF, STEPS, 100 * r) for r in range(ROUNDS)]
        ctx.train_end()
        ctx.close()
    print("WORKER " + json.dumps(out), flush=True)


def run_worker(root):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", root], capture_output=True, text=True, timeout=600,
                       cwd=root)
    line = [x for x in p.stdout.splitlines() if x.startswith("WORKER ")]
    if p.returncode != 0 or not line:
        raise RuntimeError(f"worker on {root} failed ({p.returncode}): {p.stderr[-2000:]}")
    return json.loads(line[-1][len("WORKER "):])


def off_on(ctx, torch, batch, sc, sf):
    """Step time with the flag off and on under the context's grid, alternating inside every round, and the kept share."""
    for on in (False, True):
        ctx.set_train_sample_culling(on)
        timed_steps(ctx, torch, batch, sc, sf, 5, 0)
    per = {False: [], True: []}
    ctx.read_culling()
    for r in range(ROUNDS):
        for on in (False, True):
            ctx.set_train_sample_culling(on)
            per[on].append(timed_steps(ctx, torch, batch, sc, sf, STEPS, 100 * r))
    samples, kept = ctx.read_culling()
    ctx.set_train_sample_culling(False)
    diff = np.array(per[True]) - np.array(per[False])
    return {"off": stats(per[False]), "on": stats(per[True]), "samples": samples, "kept": kept,
            "kept_share": kept / max(samples, 1), "network_passes_per_step": 2,
            "on_minus_off_ms": {"mean": float(diff.mean()), "std_of_round_differences": float(diff.std(ddof=1)),
                                "stderr": float(diff.std(ddof=1) / np.sqrt(len(diff)))},
            "on_over_off": float(np.mean(per[True]) / np.mean(per[False]))}


def main(argv):
    skip = argv.index("--parent-root") + 1 if "--parent-root" in argv else -1
    out_path = os.path.abspath(next((a for i, a in enumerate(argv) if not a.startswith("--") and i != skip),
                                    "train_culling_measure.json"))
    res = {"config": f"{N_RAYS} rays x (64+128), train_step(want_metrics=False), {ROUNDS} rounds of {STEPS} steps, one synchronise "
                     f"per round; Glorot weights except for the shipped checkpoint"}

    def save():
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)

    # ---- 1. flag off, bench.py's step: this build and, alternating with it, the parent's -------------------------------------------
    roots = [("this_commit", ROOT)] + ([("parent_commit", parent)] if parent else [])
    rounds = {name: {p: [] for p in POLICIES} for name, _ in roots}
    for _ in range(2 if parent else 1):
        for name, root in (roots[::-1] if parent else roots):
            got = run_worker(root)
            for p in POLICIES:
                rounds[name][p] += got[p]
    res["flag_off"] = {name: {p: stats(v[p]) for p in POLICIES} for name, v in rounds.items()}
    if parent:
        for p in POLICIES:
            a, b = res["flag_off"]["this_commit"][p], res["flag_off"]["parent_commit"][p]
            res["flag_off"][f"this_minus_parent_ms_{p}"] = a["ms_per_step_mean"] - b["ms_per_step_mean"]
            res["flag_off"][f"spread_ms_{p}"] = max(a["std_over_rounds"], b["std_over_rounds"])
    save()
    print(json.dumps(res["flag_off"], indent=1), flush=True)

    # ---- 2-4. flag on against off under a grid -----------------------------------------------------------------------------------------
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import bench
    import nerf_and_dietnerf_amd as N
    import occupancy_ref as G
    lo, hi = (-0.4, -0.4, -0.4), (0.4, 0.4, 0.4)
    grid128 = G.two_balls(128, np.array(lo, np.float32) * 2.5, np.array(hi, np.float32) * 2.5) | \
        (np.random.default_rng(1).random((128, 128, 128)) < 0.02)
    g = np.load(os.path.join(ROOT, "tests", "golden", "alexander50_epoch095.npz"))
    batch = bench_batch(torch)
    for policy in POLICIES:
        entry = {}
        ctx = N.Context(near=bench.NEAR, far=bench.FAR, precision="f16x3")
        ctx.load_weights(0, N.glorot_blob(0)); ctx.load_weights(1, N.glorot_blob(1))
        ctx.set_scene_box(lo, hi)
        ctx.train_begin(5e-4, mixed_float16=policy == "mixed_float16")
        for name, grid in (("full_grid", np.ones((128, 128, 128), bool)), ("synthetic_grid", grid128)):
            ctx.set_occupancy_grid(grid)
            entry[name] = dict(grid_fill=float(grid.mean()), box=[lo, hi], **off_on(ctx, torch, batch, bench.SC, bench.SF))
        ctx.train_end()
        ctx.close()
        # the shipped checkpoint: its two golden cameras' rays (2 x 50 x 50, the first 4096), targets from the golden images
        near, far, fov = float(g["near"]), float(g["far"]), float(g["fov"])
        ctx = N.Context(near=near, far=far, precision="f16x3")
        ctx.load_weights(0, g["blob_coarse"]); ctx.load_weights(1, g["blob_fine"])
        box = ((-1.5, -1.5, -2.2), (1.5, 1.5, 0.5))
        ctx.set_scene_box(*box)
        count = ctx.bake_occupancy_grid(1, 64, 5.0, samples_per_cell=2, dilate=1)
        o, d, t = [], [], []
        for cam in ("train", "test"):
            c2w = torch.as_tensor(g["c2w_" + cam], device="cuda")
            dirs = ctx.get_rays_directions(50, 50, fov, c2w).reshape(-1, 4)
            o.append(c2w[:, 3].expand(dirs.shape[0], 4)); d.append(dirs)
            t.append(torch.as_tensor(g["img_" + cam].astype(np.float32) / 255.0, device="cuda").reshape(-1, 3))
        ship = tuple(torch.cat(x)[:N_RAYS].contiguous() for x in (o, d, t))
        ctx.train_begin(5e-4, mixed_float16=policy == "mixed_float16")
        entry["shipped_checkpoint"] = dict(grid_fill=count / 64 ** 3, box=box, **off_on(ctx, torch, ship, 64, 128))
        ctx.train_end()
        ctx.close()
        res[policy] = entry
        save()
        print(policy, json.dumps(entry, indent=1), flush=True)
    print("done", flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--worker":
        worker(sys.argv[2])
    else:
        parent = os.path.abspath(sys.argv[sys.argv.index("--parent-root") + 1]) if "--parent-root" in sys.argv else None
        main(sys.argv[1:])
