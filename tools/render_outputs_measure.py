"""Measurements for the differentiable render outputs (nerf_train_render_forward_outputs / _backward_outputs; DESIGN.md 7.3,
profiles/render_outputs_measure.json), on one MI355X, at the shape of DietNeRF's consistency render: 2048 rays x (55 + 55), both
policies, device tensors in and out, forward + backward pairs through one slot enqueued back to back, one synchronise at the
end of a round:

1. the EXISTING entry points (nerf_train_render_forward / _backward, d_rgb only).  With --parent-root DIR (a checkout of the
   parent commit, built) the same loop runs on the parent's library too, in processes of their own that alternate with this
   build's, so that the old calls can be held to the parent's within the round-to-round spread;
2. the new entry points with all four outputs and all four cotangents against the old ones, alternating inside every round
   on one context: mean and standard error of the round differences;
3. nerf_render_output_grads on device arrays of the last pass's shape (2048 x 110), all three cotangents, both outputs: per call
   enqueued back to back (so the figure holds the launch), and per 2048 rays inside one launch of 32 x 2048 rays.

    python tools/render_outputs_measure.py [OUT.json] [--parent-root DIR]"""
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


def batch_of(torch):
    """bench.py's kind of rays, and 0.1 N(0, 1) cotangents for every output."""
    gen = torch.Generator(device="cuda").manual_seed(0)
    o = torch.zeros((N_RAYS, 4), device="cuda"); o[:, 2] = 1.0; o[:, 3] = 1.0
    d = torch.randn((N_RAYS, 4), device="cuda", generator=gen) * 0.3; d[:, 2] = -1.0; d[:, 3] = 0.0
    cot = {k: torch.randn(s, device="cuda", generator=gen) * 0.1
           for k, s in (("d_rgb", (N_RAYS, 3)), ("d_depth", (N_RAYS,)), ("d_weights", (N_RAYS, SC + SF)), ("d_z", (N_RAYS, SC + SF)))}
    return o, d, cot


def pair_old(ctx, o, d, cot, seed):
    ctx.train_render_forward(0, o, d, SC, SF, seed=seed)
    ctx.train_render_backward(0, cot["d_rgb"], want_blobs=False)


def pair_new(ctx, o, d, cot, seed):
    ctx.train_render_forward_outputs(0, o, d, SC, SF, seed=seed)
    ctx.train_render_backward_outputs(0, **cot, want_blobs=False)


def timed_pairs(ctx, torch, pair, o, d, cot, pairs, seed0):
    torch.cuda.synchronize()
    ctx.synchronize()
    t0 = time.perf_counter()
    for i in range(pairs):
        pair(ctx, o, d, cot, seed0 + i)
    ctx.synchronize()
    return (time.perf_counter() - t0) / pairs * 1e3


def new_trainer(N, bench, policy):
    ctx = N.Context(near=bench.NEAR, far=bench.FAR, precision="f16x3")
    ctx.load_weights(0, N.glorot_blob(0)); ctx.load_weights(1, N.glorot_blob(1))
    ctx.train_begin(5e-4, mixed_float16=policy == "mixed_float16")
    return ctx


def worker(root):
    """Setting 1 on the package under `root`: per policy, ROUNDS rounds of PAIRS pairs of the old calls -> one JSON line."""
    sys.path.insert(0, root)
    import torch
    import bench
    import nerf_and_dietnerf_amd as N
    assert os.path.realpath(os.path.dirname(N.__file__)).startswith(os.path.realpath(root)), N.__file__
    o, d, cot = batch_of(torch)
    out = {}
    for policy in POLICIES:
        ctx = new_trainer(N, bench, policy)
        timed_pairs(ctx, torch, pair_old, o, d, cot, 5, 0)
        out[policy] = [timed_pairs(ctx, torch, pair_old, o, d, cot, PAIRS, 100 * r) for r in range(ROUNDS)]
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


def old_new(ctx, torch, o, d, cot):
    """A pair through the old calls (d_rgb) and through the new ones (four outputs, four cotangents), alternating inside every round."""
    for pair in (pair_old, pair_new):
        timed_pairs(ctx, torch, pair, o, d, cot, 5, 0)
    per = {"old": [], "new": []}
    for r in range(ROUNDS):
        for name, pair in (("old", pair_old), ("new", pair_new)):
            per[name].append(timed_pairs(ctx, torch, pair, o, d, cot, PAIRS, 100 * r))
    diff = np.array(per["new"]) - np.array(per["old"])
    return {"old_d_rgb_only": stats(per["old"]), "new_four_outputs_four_cotangents": stats(per["new"]),
            "new_minus_old_ms": {"mean": float(diff.mean()), "std_of_round_differences": float(diff.std(ddof=1)),
                                 "stderr": float(diff.std(ddof=1) / np.sqrt(len(diff)))},
            "new_over_old": float(np.mean(per["new"]) / np.mean(per["old"]))}


def kernel_time(ctx, torch, s, calls=200, fold=32):
    """nerf_render_output_grads on device arrays (N_RAYS x s), microseconds: per back-to-back call, and per N_RAYS rays of one
    launch over fold x N_RAYS rays."""
    gen = torch.Generator(device="cuda").manual_seed(s)
    out = {}
    for name, n in (("per_call_us", N_RAYS), (f"per_{N_RAYS}_rays_in_a_large_launch_us", N_RAYS * fold)):
        w, z, dw, dz = (torch.rand((n, s), device="cuda", generator=gen) for _ in range(4))
        dd = torch.rand((n,), device="cuda", generator=gen)
        reps = calls if n == N_RAYS else 20
        rounds = []
        for _ in range(5):
            ctx.render_output_grads(w, z, dd, dw, dz)
            torch.cuda.synchronize(); ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                ctx.render_output_grads(w, z, dd, dw, dz)
            ctx.synchronize()
            rounds.append((time.perf_counter() - t0) / reps * 1e6 / (n // N_RAYS))
        out[name] = {"mean": float(np.mean(rounds)), "min": float(np.min(rounds)), "per_round": np.round(rounds, 3).tolist()}
    out[f"bytes_per_{N_RAYS}_rays"] = N_RAYS * s * 4 * 6 + N_RAYS * 4      # w, z, d_w, d_z read, g_w, g_z written; d_depth
    return out


def main(argv):
    skip = argv.index("--parent-root") + 1 if "--parent-root" in argv else -1
    out_path = os.path.abspath(next((a for i, a in enumerate(argv) if not a.startswith("--") and i != skip),
                                    "render_outputs_measure.json"))
    res = {"config": f"{N_RAYS} rays x ({SC}+{SF}), forward + backward pairs through one slot, device tensors, no blob copies, "
                     f"{ROUNDS} rounds of {PAIRS} pairs, one synchronise per round; Glorot weights"}

    def save():
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)

    # ---- 1. the old calls: this build and, alternating with it, the parent's ---------------------------------------------------------
    roots = [("this_commit", ROOT)] + ([("parent_commit", parent)] if parent else [])
    rounds = {name: {p: [] for p in POLICIES} for name, _ in roots}
    for _ in range(2 if parent else 1):
        for name, root in (roots[::-1] if parent else roots):
            got = run_worker(root)
            for p in POLICIES:
                rounds[name][p] += got[p]
    res["old_entry_points"] = {name: {p: stats(v[p]) for p in POLICIES} for name, v in rounds.items()}
    if parent:
        for p in POLICIES:
            a, b = res["old_entry_points"]["this_commit"][p], res["old_entry_points"]["parent_commit"][p]
            res["old_entry_points"][f"this_minus_parent_ms_{p}"] = a["ms_per_pair_mean"] - b["ms_per_pair_mean"]
            res["old_entry_points"][f"spread_ms_{p}"] = max(a["std_over_rounds"], b["std_over_rounds"])
    save()
    print(json.dumps({k: v for k, v in res["old_entry_points"].items() if k.startswith(("this_minus", "spread"))}, indent=1), flush=True)

    # ---- 2. new against old; 3. the kernel ---------------------------------------------------------------------------------------------
    sys.path.insert(0, ROOT)
    import torch
    import bench
    import nerf_and_dietnerf_amd as N
    o, d, cot = batch_of(torch)
    for policy in POLICIES:
        ctx = new_trainer(N, bench, policy)
        res[policy] = old_new(ctx, torch, o, d, cot)
        ctx.train_end()
        ctx.close()
        save()
        print(policy, json.dumps(res[policy]["new_minus_old_ms"]), res[policy]["new_over_old"], flush=True)
    ctx = N.Context(near=bench.NEAR, far=bench.FAR, precision="f16x3")
    res["fold_kernel"] = {f"{N_RAYS}x{SC + SF}": kernel_time(ctx, torch, SC + SF)}
    ctx.close()
    save()
    print(json.dumps(res["fold_kernel"], indent=1), flush=True)
    print("done", flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--worker":
        worker(sys.argv[2])
    else:
        parent = os.path.abspath(sys.argv[sys.argv.index("--parent-root") + 1]) if "--parent-root" in sys.argv else None
        main(sys.argv[1:])
