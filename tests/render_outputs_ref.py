"""References for the differentiable render outputs (nerf_train_render_forward_outputs / _backward_outputs) -- test
infrastructure only.

fold: the numpy float32 restatement of the one new kernel (render_output_fold_kernel), every operation rounded on its own.
render_outputs_gradients: oracle.train_oracle.render_gradients' graph with all four outputs of the last pass and a cotangent
for each, L = sum(d_rgb rgb) + sum(d_depth depth) + sum(d_weights w) + sum(d_z z), by torch-CPU autograd.
"""
import numpy as np
import torch

from oracle import nerf_oracle as O
from oracle import train_oracle as T


def fold(weights, z, d_depth=None, d_weights=None, d_z=None):
    """g_w = d_weights + d_depth * z, g_z = d_z + d_depth * weights in float32 (numpy rounds the product, then the sum); an
    absent input counts as 0.  -> (g_w, g_z), each (N, S)."""
    w, z = np.asarray(weights, np.float32), np.asarray(z, np.float32)
    zero = np.zeros(w.shape, np.float32)
    dw = zero if d_weights is None else np.asarray(d_weights, np.float32)
    dz = zero if d_z is None else np.asarray(d_z, np.float32)
    if d_depth is None:
        pz, pw = zero, zero
    else:
        dd = np.asarray(d_depth, np.float32)[:, None]
        pz, pw = (dd * z).astype(np.float32), (dd * w).astype(np.float32)
    return (dw + pz).astype(np.float32), (dz + pw).astype(np.float32)


def render_outputs_forward(pc, pf, rays_o, rays_d, near, far, u_c, u_f, n_xyz=5, n_dir=4, n_angles=2, alpha=0.05,
                           sampler_grad=True, dtype=torch.float64, fp16_loss_scale=None):
    """The graph of T.render_gradients, statement by statement, keeping what it drops: -> (rgb, depth, weights, z) of the
    last pass as torch tensors with the graph attached."""
    o = torch.tensor(np.asarray(rays_o), dtype=dtype)
    d = torch.tensor(np.asarray(rays_d), dtype=dtype)
    z = torch.tensor(O.get_z_values(near, far, np.asarray(u_c, np.float32)), dtype=dtype)
    rgb, w = T._render_rays(pc, o, d, z, n_xyz, n_dir, n_angles, alpha, fp16_loss_scale)
    if pf is not None:
        z_f = T._sample_pdf(w if sampler_grad else w.detach(), z, torch.tensor(np.asarray(u_f), dtype=dtype))
        z = torch.sort(torch.cat([z_f, z], -1), -1).values
        rgb, w = T._render_rays(pf, o, d, z, n_xyz, n_dir, n_angles, alpha, fp16_loss_scale)
    return rgb, (w * z).sum(-1), w, z


def render_outputs_gradients(blob_c, blob_f, rays_o, rays_d, near, far, u_c, u_f, d_rgb=None, d_depth=None, d_weights=None,
                             d_z=None, dtype=torch.float64, **kw):
    """Autograd of L = sum(d_rgb rgb) + sum(d_depth depth) + sum(d_weights weights) + sum(d_z z) (absent cotangents: 0).
    Keywords as T.render_gradients (n_pos_enc_xyz, n_pos_enc_dir, n_angles, alpha, sampler_grad, fp16_loss_scale).
    -> dict(rgb, depth, weights, z, loss, grad_coarse, grad_fine | None)."""
    shape_kw = {k: kw[k] for k in ("n_pos_enc_xyz", "n_pos_enc_dir", "n_angles") if k in kw}
    pc = T.blob_to_params(blob_c, dtype, **shape_kw)
    pf = T.blob_to_params(blob_f, dtype, **shape_kw) if blob_f is not None else None
    outs = render_outputs_forward(pc, pf, rays_o, rays_d, near, far, u_c, u_f, kw.get("n_pos_enc_xyz", 5),
                                  kw.get("n_pos_enc_dir", 4), kw.get("n_angles", 2), kw.get("alpha", 0.05),
                                  kw.get("sampler_grad", True), dtype, kw.get("fp16_loss_scale"))
    loss = _loss(outs, (d_rgb, d_depth, d_weights, d_z), dtype)
    if loss.requires_grad:        # (d_z alone on a coarse-only render: z is data, the gradient is zero)
        loss.backward()
    g = lambda ps: np.concatenate([(t.grad if t.grad is not None else torch.zeros_like(t)).numpy().ravel() for t in ps])
    rgb, depth, w, z = (t.detach().numpy() for t in outs)
    return dict(rgb=rgb, depth=depth, weights=w, z=z, loss=float(loss.detach()), grad_coarse=g(pc),
                grad_fine=g(pf) if pf is not None else None)


def _loss(outs, cots, dtype):
    loss = None
    for out, cot in zip(outs, cots):
        if cot is not None:
            term = (out * torch.tensor(np.asarray(cot), dtype=dtype)).sum()
            loss = term if loss is None else loss + term
    assert loss is not None, "at least one cotangent"
    return loss


def render_outputs_gradient_sets(blob_c, blob_f, rays_o, rays_d, near, far, u_c, u_f, sets, dtype=torch.float64, **kw):
    """render_outputs_gradients for several cotangent sets on ONE forward graph (the forward is the expensive half and does
    not depend on the cotangents).  sets: {name: dict of d_rgb / d_depth / d_weights / d_z}.
    -> dict(rgb, depth, weights, z, grads={name: (grad_coarse, grad_fine | None)})."""
    shape_kw = {k: kw[k] for k in ("n_pos_enc_xyz", "n_pos_enc_dir", "n_angles") if k in kw}
    pc = T.blob_to_params(blob_c, dtype, **shape_kw)
    pf = T.blob_to_params(blob_f, dtype, **shape_kw) if blob_f is not None else None
    outs = render_outputs_forward(pc, pf, rays_o, rays_d, near, far, u_c, u_f, kw.get("n_pos_enc_xyz", 5),
                                  kw.get("n_pos_enc_dir", 4), kw.get("n_angles", 2), kw.get("alpha", 0.05),
                                  kw.get("sampler_grad", True), dtype, kw.get("fp16_loss_scale"))
    params = pc + (pf or [])
    grads = {}
    for name, cot in sets.items():
        loss = _loss(outs, [cot.get(k) for k in ("d_rgb", "d_depth", "d_weights", "d_z")], dtype)
        if loss.requires_grad:
            gs = torch.autograd.grad(loss, params, retain_graph=True, allow_unused=True)
        else:
            gs = [None] * len(params)
        flat = [(g if g is not None else torch.zeros_like(t)).numpy().ravel() for g, t in zip(gs, params)]
        grads[name] = (np.concatenate(flat[:len(pc)]), np.concatenate(flat[len(pc):]) if pf is not None else None)
    rgb, depth, w, z = (t.detach().numpy() for t in outs)
    return dict(rgb=rgb, depth=depth, weights=w, z=z, grads=grads)


# ---- what tests/test_gpu_render_outputs.py and tests/test_gpu_ray_gradients.py both draw and call --------------------------------
NAMES = ("d_rgb", "d_depth", "d_weights", "d_z")


def cotangents(n, s, seed=3):
    """0.1 N(0, 1) for each of the four outputs; d_rgb is drawn first, as test_backward_through_render draws its own."""
    rng = np.random.default_rng(seed)
    shapes = {"d_rgb": (n, 3), "d_depth": (n,), "d_weights": (n, s), "d_z": (n, s)}
    return {k: (rng.standard_normal(shapes[k]) * 0.1).astype(np.float32) for k in NAMES}


def draws(p):
    return (p["sc"], p["sf"], p["u_c"], p["u_f"])


def forward(ctx, p, slot=0, **kw):
    return ctx.train_render_forward_outputs(slot, p["o"], p["d"], *draws(p), **kw)
