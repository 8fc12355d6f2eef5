"""Measurements for the distortion regulariser of the trainer (nerf_train_set_distortion_weights; DESIGN.md 1.2,
profiles/distortion_measure.json), on one MI355X: the training step bench.py times -- 4096 rays x (64+128), both policies,
train_step(want_metrics=False) enqueued back to back, one synchronise at the end of a round -- and the kernel by itself:

1. both weights 0: bench.py's own figure.  With --parent-root DIR (a checkout of the parent commit, built) the same loop runs on
   the parent's library too, in processes of their own that alternate with this build's, so that the step without the regulariser
   can be held to the parent's within the round-to-round spread;
2. weights (0.01, 0.01) against (0, 0), alternating inside every round on one context;
3. nerf_distortion_loss on device arrays of the two passes' shapes (4096 x 64, 4096 x 128), all three outputs: per call as the
   trainer launches it (enqueued back to back, so the figure holds the launch), and per 4096 rays inside one launch of 32 x 4096
   rays (the kernel's own rate).

    python tools/distortion_measure.py [OUT.json] [--parent-root DIR]"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))       # the repository: this file lives in tools/
N_RAYS, ROUNDS, STEPS = 4096, 10, 20
POLICIES = ("float32", "mixed_float16")
WEIGHTS = (0.01, 0.01)


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


def new_trainer(N, bench, policy):
    ctx = N.Context(near=bench.NEAR, far=bench.FAR, precision="f16x3")
    ctx.load_weights(0, N.glorot_blob(0)); ctx.load_weights(1, N.glorot_blob(1))
    ctx.train_begin(5e-4, mixed_float16=policy == "mixed_float16")
    return ctx


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
        ctx = new_trainer(N, bench, policy)
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
    """Step time with the weights at (0, 0) and at WEIGHTS, alternating inside every round."""
    for w in ((0.0, 0.0), WEIGHTS):
        ctx.train_set_distortion_weights(*w)
        timed_steps(ctx, torch, batch, sc, sf, 5, 0)
    per = {False: [], True: []}
    ctx.train_read_distortion_sums()
    for r in range(ROUNDS):
        for on in (False, True):
            ctx.train_set_distortion_weights(*(WEIGHTS if on else (0.0, 0.0)))
            per[on].append(timed_steps(ctx, torch, batch, sc, sf, STEPS, 100 * r))
    sums, steps = ctx.train_read_distortion_sums()
    diff = np.array(per[True]) - np.array(per[False])
    return {"off": stats(per[False]), "on": stats(per[True]), "weights": list(WEIGHTS),
            "mean_distortion": {k: v / max(steps, 1) for k, v in sums.items()}, "steps_under_the_regulariser": steps,
            "on_minus_off_ms": {"mean": float(diff.mean()), "std_of_round_differences": float(diff.std(ddof=1)),
                                "stderr": float(diff.std(ddof=1) / np.sqrt(len(diff)))},
            "on_over_off": float(np.mean(per[True]) / np.mean(per[False]))}


def kernel_time(ctx, torch, s, calls=200, fold=32):
    """nerf_distortion_loss on device arrays (N_RAYS x s), microseconds: per back-to-back call, and per N_RAYS rays of one
    launch over fold x N_RAYS rays."""
    gen = torch.Generator(device="cuda").manual_seed(s)
    out = {}
    for name, n in (("per_call_us", N_RAYS), ("per_4096_rays_in_a_large_launch_us", N_RAYS * fold)):
        alpha = torch.rand((n, s), device="cuda", generator=gen) * (2.0 / s ** 0.5)
        w = alpha * torch.cumprod(torch.cat([torch.ones((n, 1), device="cuda"), 1.0 - alpha[:, :-1]], -1), -1)
        z = ctx.cfg.near_boundary + (ctx.cfg.far_boundary - ctx.cfg.near_boundary) * \
            (torch.arange(s, device="cuda")[None, :] + torch.rand((n, s), device="cuda", generator=gen)) / s
        w, z = w.contiguous(), z.contiguous()
        reps = calls if n == N_RAYS else 20
        rounds = []
        for _ in range(5):
            ctx.distortion_loss(w, z)
            torch.cuda.synchronize(); ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                ctx.distortion_loss(w, z)
            ctx.synchronize()
            rounds.append((time.perf_counter() - t0) / reps * 1e6 / (n // N_RAYS))
        out[name] = {"mean": float(np.mean(rounds)), "min": float(np.min(rounds)), "per_round": np.round(rounds, 3).tolist()}
    out["bytes_per_4096_rays"] = N_RAYS * s * 4 * 4 + N_RAYS * 4        # w, z read; d_w, d_z, L_ray written (the second sweep's
    return out                                                          # re-read of w and z comes out of the cache)


def main(argv):
    skip = argv.index("--parent-root") + 1 if "--parent-root" in argv else -1
    out_path = os.path.abspath(next((a for i, a in enumerate(argv) if not a.startswith("--") and i != skip),
                                    "distortion_measure.json"))
    res = {"config": f"{N_RAYS} rays x (64+128), train_step(want_metrics=False), {ROUNDS} rounds of {STEPS} steps, one synchronise "
                     f"per round; Glorot weights"}

    def save():
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)

    # ---- 1. both weights 0, bench.py's step: this build and, alternating with it, the parent's ------------------------------------
    roots = [("this_commit", ROOT)] + ([("parent_commit", parent)] if parent else [])
    rounds = {name: {p: [] for p in POLICIES} for name, _ in roots}
    for _ in range(2 if parent else 1):
        for name, root in (roots[::-1] if parent else roots):
            got = run_worker(root)
            for p in POLICIES:
                rounds[name][p] += got[p]
    res["weights_zero"] = {name: {p: stats(v[p]) for p in POLICIES} for name, v in rounds.items()}
    if parent:
        for p in POLICIES:
            a, b = res["weights_zero"]["this_commit"][p], res["weights_zero"]["parent_commit"][p]
            res["weights_zero"][f"this_minus_parent_ms_{p}"] = a["ms_per_step_mean"] - b["ms_per_step_mean"]
            res["weights_zero"][f"spread_ms_{p}"] = max(a["std_over_rounds"], b["std_over_rounds"])
    save()
    print(json.dumps(res["weights_zero"], indent=1), flush=True)

    # ---- 2. the regulariser on against off; 3. the kernel -----------------------------------------------------------------------------
    sys.path.insert(0, ROOT)
    import torch
    import bench
    import nerf_and_dietnerf_amd as N
    batch = bench_batch(torch)
    for policy in POLICIES:
        ctx = new_trainer(N, bench, policy)
        res[policy] = off_on(ctx, torch, batch, bench.SC, bench.SF)
        ctx.train_end()
        ctx.close()
        save()
        print(policy, json.dumps(res[policy], indent=1), flush=True)
    ctx = N.Context(near=bench.NEAR, far=bench.FAR, precision="f16x3")
    res["kernel"] = {f"{N_RAYS}x{s}": kernel_time(ctx, torch, s) for s in (bench.SC, bench.SF)}
    ctx.close()
    save()
    print(json.dumps(res["kernel"], indent=1), flush=True)
    print("done", flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--worker":
        worker(sys.argv[2])
    else:
        parent = os.path.abspath(sys.argv[sys.argv.index("--parent-root") + 1]) if "--parent-root" in sys.argv else None
        main(sys.argv[1:])
