"""Measurements for the encoding window (nerf_ctx_set_encoding_window; README "Coarse-to-fine positional encoding",
profiles/encoding_window_measure.json), on one MI355X:

(a) the window OFF against the parent commit: with --parent-root DIR (a checkout of the parent commit, built) bench.py's
    frame (three rounds of ten frames) and the 4096 x (64 + 128) training step under both policies (ten rounds of twenty
    steps) run on the parent's library too, in processes of their own that alternate with this build's -- the feature is
    meant to cost nothing while it is off;
(b) on one trainer per policy, alternating inside every round (which goes first takes turns): the step with the window off | on (the re-pack reads one more
    table, the reductions of four layers one more factor), and the time of one set_encoding_window call with the trainer
    running (two windows taking turns, enqueued back to back, one synchronise per round);
(c) one demonstration, recorded and not barred: the README's pose refinement (golden test pose, weights frozen, torch Adam at
    1e-3 on the translation, 48 rays x (16 + 24)) from an offset of 0.1 per axis, once with the full-band encoding and once
    with set_encoding_alpha opened linearly from 0 to L over the steps: final photometric loss (full band) and translation
    error of both.

    python tools/encoding_window_measure.py [OUT.json] [--parent-root DIR]"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))       # the repository: this file lives in tools/
N_RAYS, SC, SF, ROUNDS, STEPS = 4096, 64, 128, 10, 20
FRAME_ROUNDS, FRAMES = 3, 10
POLICIES = ("float32", "mixed_float16")
POSE_STEPS, POSE_OFFSET = 200, 0.1


def stats(a):
    a = np.asarray(a, np.float64)
    return {"ms_mean": float(a.mean()), "std_over_rounds": float(a.std(ddof=1)), "min": float(a.min()), "max": float(a.max()),
            "per_round_ms": a.round(4).tolist()}


def diff_stats(a, b):
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return {"mean": float(d.mean()), "std_of_round_differences": float(d.std(ddof=1)), "stderr": float(d.std(ddof=1) / np.sqrt(len(d)))}


def batch_of(torch):
    """bench.py's kind of rays and random targets."""
    gen = torch.Generator(device="cuda").manual_seed(0)
    o = torch.zeros((N_RAYS, 4), device="cuda"); o[:, 2] = 1.0; o[:, 3] = 1.0
    d = torch.randn((N_RAYS, 4), device="cuda", generator=gen) * 0.3; d[:, 2] = -1.0; d[:, 3] = 0.0
    return o, d, torch.rand((N_RAYS, 3), device="cuda", generator=gen)


def timed_steps(ctx, torch, batch, steps, seed0):
    torch.cuda.synchronize()
    ctx.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        ctx.train_step(*batch, SC, SF, seed=seed0 + i, want_metrics=False)
    ctx.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def new_trainer(N, bench, policy):
    ctx = N.Context(near=bench.NEAR, far=bench.FAR, precision="f16x3")
    ctx.load_weights(0, N.glorot_blob(0)); ctx.load_weights(1, N.glorot_blob(1))
    ctx.train_begin(5e-4, mixed_float16=policy == "mixed_float16")
    return ctx


def worker(root):
    """Setting (a) on the package under `root` (the window never set) -> one JSON line."""
    sys.path.insert(0, root)
    import torch
    import bench
    import nerf_and_dietnerf_amd as N
    assert os.path.realpath(os.path.dirname(N.__file__)).startswith(os.path.realpath(root)), N.__file__
    out = {}
    net_cfg = {"hidden_layer_dim": 256, "last_hidden_layer_dim": 128, "leaky_relu_alpha": 0.05, "n_pos_enc_dim_xyz": 5,
               "n_pos_enc_view_dir": 4, "n_angles_for_model": 2, "n_rays_in_batch_train": 4096, "n_rays_in_batch_render": 4096}
    model = N.NeRF(net_cfg, {"n_render_samples_coarse": bench.SC, "n_render_samples_fine": bench.SF}, bench.NEAR, bench.FAR,
                   precision="f16x3")
    model.set_weights(N.glorot_blob(0), N.glorot_blob(1))
    c2w = bench.sphere_matrix(1.0, -30.0, 45.0, 0.0)

    def frames(n, seed0):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            model.render_image(c2w, bench.FOV, bench.H, bench.W, batch_size_input=1 << 18, seed=seed0 + i, device_out=True,
                               rgb_only=True)
        model.ctx.synchronize()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3
    frames(2, 0)
    out["frame"] = [frames(FRAMES, 10 * (r + 1)) for r in range(FRAME_ROUNDS)]
    model.ctx.close()
    batch = batch_of(torch)
    for policy in POLICIES:
        ctx = new_trainer(N, bench, policy)
        timed_steps(ctx, torch, batch, 5, 0)
        out[policy] = [timed_steps(ctx, torch, batch, STEPS, 100 * (r + 1)) for r in range(ROUNDS)]
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


def off_on(ctx, torch, batch, windows):
    """Setting (b): window off | on, alternating inside every round; then the set call itself."""
    modes = (("off", (None, None)), ("on", windows[0]))
    for _, w in modes:
        ctx.set_encoding_window(*w)
        timed_steps(ctx, torch, batch, 5, 0)
    per = {name: [] for name, _ in modes}
    for r in range(ROUNDS):
        for name, w in (modes if r % 2 == 0 else modes[::-1]):      # (which runs first takes turns: an order effect cancels)
            ctx.set_encoding_window(*w)
            per[name].append(timed_steps(ctx, torch, batch, STEPS, 100 * (r + 1)))
    calls = []
    for r in range(ROUNDS):
        ctx.synchronize()
        t0 = time.perf_counter()
        for i in range(STEPS):
            ctx.set_encoding_window(*windows[i % 2])
        ctx.synchronize()
        calls.append((time.perf_counter() - t0) / STEPS * 1e3)
    ctx.set_encoding_window(None, None)
    return {**{name: stats(v) for name, v in per.items()}, "on_minus_off_ms": diff_stats(per["on"], per["off"]),
            "on_over_off": float(np.mean(per["on"]) / np.mean(per["off"])), "set_encoding_window_call_ms": stats(calls)}


def pose_demo(N, torch):
    """Setting (c) -> {"full_band": ..., "windowed": ...}: losses are full-band photometric losses against the true pose's render."""
    ck = np.load(os.path.join(ROOT, "tests", "golden", "alexander50_epoch095.npz"))
    hw, n, sc, sf, L = 16, 48, 16, 24, 5
    fov = float(ck["fov"])
    out = {}
    for name in ("full_band", "windowed"):
        ctx = N.Context(near=float(ck["near"]), far=float(ck["far"]), precision="fp32")
        ctx.load_weights(0, ck["blob_coarse"]); ctx.load_weights(1, ck["blob_fine"])
        ctx.train_begin(5e-4)
        ctx.train_set_ray_gradients(True)
        c2w = torch.as_tensor(ck["c2w_test"].astype(np.float32), device="cuda")
        rs = np.random.default_rng(0)
        idx = torch.as_tensor(rs.choice(hw * hw, n, replace=False), device="cuda")
        u_c = torch.as_tensor(rs.random((n, sc), dtype=np.float32), device="cuda")
        u_f = torch.as_tensor(rs.random((n, sf), dtype=np.float32), device="cuda")
        render = lambda o, d: N.render_with_grad(ctx, o, d, sc, sf, u_coarse=u_c, u_fine=u_f)["rgb"]     # noqa: E731

        def full_band_loss(pose, target=None):
            """The photometric loss without a window (a forward alone leaves its slot held: released before the window moves)."""
            keep = ctx.encoding_window()
            ctx.train_render_release()
            ctx.set_encoding_window(None, None)
            with torch.no_grad():
                rgb = render(*N.rays_from_pose(pose, fov, hw, hw, idx)).clone()
            ctx.train_render_release()
            if keep is not None:
                ctx.set_encoding_window(*keep)
            return rgb if target is None else float(((rgb - target) ** 2).mean())
        target = full_band_loss(c2w)
        trans = torch.nn.Parameter(c2w[:3, 3] + torch.full((3,), POSE_OFFSET, device="cuda"))
        opt = torch.optim.Adam([trans], lr=1e-3)
        pose_of = lambda: torch.cat([c2w[:, :3], torch.cat([trans, c2w[3:, 3]])[:, None]], 1)      # noqa: E731
        first = full_band_loss(pose_of().detach(), target)
        err0 = float((trans.detach() - c2w[:3, 3]).norm())
        trace = []
        for step in range(POSE_STEPS):
            if name == "windowed":
                alpha = L * step / (POSE_STEPS - 1)
                ctx.set_encoding_window(N.encoding_window(alpha, L, "linear"), None)
            loss = ((render(*N.rays_from_pose(pose_of(), fov, hw, hw, idx)) - target) ** 2).mean()
            opt.zero_grad()
            loss.backward()
            opt.step()
            if step % 20 == 19:
                trace.append(round(float((trans.detach() - c2w[:3, 3]).norm()), 5))
        assert name == "full_band" or ctx.encoding_window() is None          # alpha reached L: the window is off
        out[name] = {"photometric_loss_first": first, "photometric_loss_last": full_band_loss(pose_of().detach(), target),
                     "translation_error_first": err0, "translation_error_last": float((trans.detach() - c2w[:3, 3]).norm()),
                     "translation_error_every_20_steps": trace}
        ctx.close()
    out["config"] = (f"golden test pose, translation offset {POSE_OFFSET} per axis, weights frozen, torch Adam 1e-3 on the translation, "
                     f"48 rays x (16 + 24), {POSE_STEPS} steps; windowed: linear window, alpha from 0 to {L} over the steps")
    return out


def main(argv, parent):
    skip = argv.index("--parent-root") + 1 if "--parent-root" in argv else -1
    out_path = os.path.abspath(next((a for i, a in enumerate(argv) if not a.startswith("--") and i != skip),
                                    "encoding_window_measure.json"))
    res = {"config": f"frame: bench.py's, {FRAME_ROUNDS} rounds of {FRAMES}; step: {N_RAYS} rays x ({SC}+{SF}), device tensors, no "
                     f"metrics read, {ROUNDS} rounds of {STEPS} steps, one synchronise per round; Glorot weights"}

    def save():
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)

    # ---- (a) the window off: this build and, alternating with it, the parent's -----------------------------------------------------------
    keys = ("frame",) + POLICIES
    roots = [("this_commit", ROOT)] + ([("parent_commit", parent)] if parent else [])
    rounds = {name: {k: [] for k in keys} for name, _ in roots}
    for _ in range(2 if parent else 1):
        for name, root in (roots[::-1] if parent else roots):
            got = run_worker(root)
            for k in keys:
                rounds[name][k] += got[k]
    res["window_off"] = {name: {k: stats(v[k]) for k in keys} for name, v in rounds.items()}
    if parent:
        for k in keys:
            a, b = res["window_off"]["this_commit"][k], res["window_off"]["parent_commit"][k]
            res["window_off"][f"this_minus_parent_ms_{k}"] = a["ms_mean"] - b["ms_mean"]
            res["window_off"][f"spread_ms_{k}"] = max(a["std_over_rounds"], b["std_over_rounds"])
    save()
    print(json.dumps({k: v for k, v in res["window_off"].items() if k.startswith(("this_minus", "spread"))}, indent=1), flush=True)

    # ---- (b) on against off, the set call; (c) the demonstration -----------------------------------------------------------------------------
    sys.path.insert(0, ROOT)
    import torch
    import bench
    import nerf_and_dietnerf_amd as N
    batch = batch_of(torch)
    rng = np.random.default_rng(0)
    windows = [((0.1 + 0.8 * rng.random(5)).astype(np.float32), (0.1 + 0.8 * rng.random(4)).astype(np.float32)) for _ in range(2)]
    for policy in POLICIES:
        ctx = new_trainer(N, bench, policy)
        res[policy] = off_on(ctx, torch, batch, windows)
        ctx.train_end()
        ctx.close()
        save()
        print(policy, json.dumps({k: res[policy][k] for k in ("on_minus_off_ms", "on_over_off")}),
              json.dumps(res[policy]["set_encoding_window_call_ms"]["ms_mean"]), flush=True)
    res["pose_refinement"] = pose_demo(N, torch)
    save()
    print(json.dumps(res["pose_refinement"], indent=1), flush=True)
    print("done", flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--worker":
        worker(sys.argv[2])
    else:
        main(sys.argv[1:], os.path.abspath(sys.argv[sys.argv.index("--parent-root") + 1]) if "--parent-root" in sys.argv else None)
