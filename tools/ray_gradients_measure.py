"""Measurements for the ray gradients (nerf_train_set_ray_gradients / nerf_train_render_backward_rays; README "Ray gradients",
profiles/ray_gradients_measure.json), on one MI355X, at the shape of tools/render_outputs_measure.py: 2048 rays x (55 + 55),
both policies, device tensors in and out, forward + backward pairs through one slot enqueued back to back, one synchronise at
the end of a round, ten rounds of twenty pairs:

(a) the switch OFF against the parent commit: with --parent-root DIR (a checkout of the parent commit, built) the loop over
    nerf_train_render_forward_outputs / _backward_outputs (four cotangents) runs on the parent's library too, in processes of
    their own that alternate with this build's -- the feature is meant to cost nothing while it is off;
(b) on one context, alternating inside every round: switch off | switch on without ray outputs (what the coarse network's
    encoding-gradient variant of the backward chain costs) | switch on with both ray outputs (plus the two new kernels per
    pass and the two memsets): mean and standard error of the round differences;
(c) the reduction stage alone, nerf_ray_position_grads on device arrays (2048 x 110 x 3): per back-to-back call (so the figure
    holds the launch and the two memsets) and per 2048 rays inside one launch of 32 x 2048 rays.

    python tools/ray_gradients_measure.py [OUT.json] [--parent-root DIR]"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))       # the repository: this file lives in tools/
N_RAYS, SC, SF, ROUNDS, PAIRS = 2048, 55, 55, 10, 20
POLICIES = ("float32", "mixed_float16")


def stats(a):
    a = np.asarray(a, np.float64)
    return {"ms_per_pair_mean": float(a.mean()), "std_over_rounds": float(a.std(ddof=1)), "min": float(a.min()),
            "max": float(a.max()), "per_round_ms": a.round(4).tolist()}


def diff_stats(a, b):
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return {"mean": float(d.mean()), "std_of_round_differences": float(d.std(ddof=1)), "stderr": float(d.std(ddof=1) / np.sqrt(len(d)))}


def batch_of(torch):
    """bench.py's kind of rays, and 0.1 N(0, 1) cotangents for every output."""
    gen = torch.Generator(device="cuda").manual_seed(0)
    o = torch.zeros((N_RAYS, 4), device="cuda"); o[:, 2] = 1.0; o[:, 3] = 1.0
    d = torch.randn((N_RAYS, 4), device="cuda", generator=gen) * 0.3; d[:, 2] = -1.0; d[:, 3] = 0.0
    cot = {k: torch.randn(s, device="cuda", generator=gen) * 0.1
           for k, s in (("d_rgb", (N_RAYS, 3)), ("d_depth", (N_RAYS,)), ("d_weights", (N_RAYS, SC + SF)), ("d_z", (N_RAYS, SC + SF)))}
    return o, d, cot


def pair(ctx, o, d, cot, seed, want_rays=False):
    ctx.train_render_forward_outputs(0, o, d, SC, SF, seed=seed, outputs=("rgb",))
    if want_rays:
        ctx.train_render_backward_outputs(0, **cot, want_blobs=False, want_rays=True)
    else:
        ctx.train_render_backward_outputs(0, **cot, want_blobs=False)


def timed_pairs(ctx, torch, o, d, cot, pairs, seed0, want_rays=False):
    torch.cuda.synchronize()
    ctx.synchronize()
    t0 = time.perf_counter()
    for i in range(pairs):
        pair(ctx, o, d, cot, seed0 + i, want_rays)
    ctx.synchronize()
    return (time.perf_counter() - t0) / pairs * 1e3


def new_trainer(N, bench, policy):
    ctx = N.Context(near=bench.NEAR, far=bench.FAR, precision="f16x3")
    ctx.load_weights(0, N.glorot_blob(0)); ctx.load_weights(1, N.glorot_blob(1))
    ctx.train_begin(5e-4, mixed_float16=policy == "mixed_float16")
    return ctx


def worker(root):
    """Setting (a) on the package under `root`: per policy, ROUNDS rounds of PAIRS pairs with the switch off -> one JSON line."""
    sys.path.insert(0, root)
    import torch
    import bench
    import nerf_and_dietnerf_amd as N
    assert os.path.realpath(os.path.dirname(N.__file__)).startswith(os.path.realpath(root)), N.__file__
    o, d, cot = batch_of(torch)
    out = {}
    for policy in POLICIES:
        ctx = new_trainer(N, bench, policy)
        timed_pairs(ctx, torch, o, d, cot, 5, 0)
        out[policy] = [timed_pairs(ctx, torch, o, d, cot, PAIRS, 100 * r) for r in range(ROUNDS)]
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


def off_on(ctx, torch, o, d, cot):
    """Setting (b): off | on, no ray outputs | on, both ray outputs -- alternating inside every round."""
    modes = (("off", False, False), ("on_no_ray_outputs", True, False), ("on_ray_outputs", True, True))
    for _, on, rays in modes:
        ctx.train_set_ray_gradients(on)
        timed_pairs(ctx, torch, o, d, cot, 5, 0, rays)
    per = {name: [] for name, _, _ in modes}
    for r in range(ROUNDS):
        for name, on, rays in modes:
            ctx.train_set_ray_gradients(on)
            per[name].append(timed_pairs(ctx, torch, o, d, cot, PAIRS, 100 * r, rays))
    ctx.train_set_ray_gradients(False)
    return {**{name: stats(v) for name, v in per.items()},
            "on_ray_outputs_minus_off_ms": diff_stats(per["on_ray_outputs"], per["off"]),
            "coarse_encoding_gradient_variant_ms": diff_stats(per["on_no_ray_outputs"], per["off"]),
            "new_kernels_and_memsets_ms": diff_stats(per["on_ray_outputs"], per["on_no_ray_outputs"]),
            "on_over_off": float(np.mean(per["on_ray_outputs"]) / np.mean(per["off"]))}


def kernel_time(ctx, torch, s, calls=200, fold=32):
    """nerf_ray_position_grads on device arrays (N_RAYS x s x 3), microseconds: per back-to-back call, and per N_RAYS rays of
    one launch over fold x N_RAYS rays."""
    gen = torch.Generator(device="cuda").manual_seed(s)
    out = {}
    for name, n in (("per_call_us", N_RAYS), (f"per_{N_RAYS}_rays_in_a_large_launch_us", N_RAYS * fold)):
        dp = torch.randn((n, s, 3), device="cuda", generator=gen)
        z = torch.rand((n, s), device="cuda", generator=gen)
        reps = calls if n == N_RAYS else 20
        rounds = []
        for _ in range(5):
            ctx.ray_position_grads(dp, z)
            torch.cuda.synchronize(); ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                ctx.ray_position_grads(dp, z)
            ctx.synchronize()
            rounds.append((time.perf_counter() - t0) / reps * 1e6 / (n // N_RAYS))
        out[name] = {"mean": float(np.mean(rounds)), "min": float(np.min(rounds)), "per_round": np.round(rounds, 3).tolist()}
    out[f"bytes_per_{N_RAYS}_rays"] = N_RAYS * s * 4 * 4 + N_RAYS * 4 * 4 * 2      # d_points, z read; two (N, 4) outputs
    return out


def main(argv, parent):
    skip = argv.index("--parent-root") + 1 if "--parent-root" in argv else -1
    out_path = os.path.abspath(next((a for i, a in enumerate(argv) if not a.startswith("--") and i != skip),
                                    "ray_gradients_measure.json"))
    res = {"config": f"{N_RAYS} rays x ({SC}+{SF}), forward + backward pairs through one slot (four cotangents), device tensors, "
                     f"no blob copies, {ROUNDS} rounds of {PAIRS} pairs, one synchronise per round; Glorot weights"}

    def save():
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)

    # ---- (a) the switch off: this build and, alternating with it, the parent's ---------------------------------------------------------
    roots = [("this_commit", ROOT)] + ([("parent_commit", parent)] if parent else [])
    rounds = {name: {p: [] for p in POLICIES} for name, _ in roots}
    for _ in range(2 if parent else 1):
        for name, root in (roots[::-1] if parent else roots):
            got = run_worker(root)
            for p in POLICIES:
                rounds[name][p] += got[p]
    res["switch_off"] = {name: {p: stats(v[p]) for p in POLICIES} for name, v in rounds.items()}
    if parent:
        for p in POLICIES:
            a, b = res["switch_off"]["this_commit"][p], res["switch_off"]["parent_commit"][p]
            res["switch_off"][f"this_minus_parent_ms_{p}"] = a["ms_per_pair_mean"] - b["ms_per_pair_mean"]
            res["switch_off"][f"spread_ms_{p}"] = max(a["std_over_rounds"], b["std_over_rounds"])
    save()
    print(json.dumps({k: v for k, v in res["switch_off"].items() if k.startswith(("this_minus", "spread"))}, indent=1), flush=True)

    # ---- (b) on against off; (c) the reduction kernel ------------------------------------------------------------------------------------
    sys.path.insert(0, ROOT)
    import torch
    import bench
    import nerf_and_dietnerf_amd as N
    o, d, cot = batch_of(torch)
    for policy in POLICIES:
        ctx = new_trainer(N, bench, policy)
        res[policy] = off_on(ctx, torch, o, d, cot)
        ctx.train_end()
        ctx.close()
        save()
        print(policy, json.dumps({k: res[policy][k] for k in ("on_ray_outputs_minus_off_ms", "coarse_encoding_gradient_variant_ms",
                                                              "new_kernels_and_memsets_ms", "on_over_off")}), flush=True)
    ctx = N.Context(near=bench.NEAR, far=bench.FAR, precision="f16x3")
    res["reduce_kernel"] = {f"{N_RAYS}x{SC + SF}x3": kernel_time(ctx, torch, SC + SF)}
    ctx.close()
    save()
    print(json.dumps(res["reduce_kernel"], indent=1), flush=True)
    print("done", flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--worker":
        worker(sys.argv[2])
    else:
        main(sys.argv[1:], os.path.abspath(sys.argv[sys.argv.index("--parent-root") + 1]) if "--parent-root" in sys.argv else None)
