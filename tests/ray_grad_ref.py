"""References for the ray gradients (nerf_train_render_backward_rays, nerf_ray_position_grads) -- test infrastructure only.

ray_gradient_sets: the graph of render_outputs_ref.render_outputs_forward with the rays as leaf tensors that require grad,
L = sum(d_rgb rgb) + sum(d_depth depth) + sum(d_weights w) + sum(d_z z), by torch-CPU autograd -> dL/d(rays_orig),
dL/d(rays_dirs) (N,4) in float64, float32 or the fp16-emulating mode.  `view_term=False` drops the view-direction input from
the graph and `sampler_grad=False` the sampler term, so a test can show how much each carries.
position_reduce: the numpy float64 restatement of the bare per-ray reduction.
"""
import numpy as np
import torch

from oracle import nerf_oracle as O
from oracle import train_oracle as T

import render_outputs_ref as R


def position_reduce(d_points, z):
    """d_points (N,S,3), z (N,S) -> (d_o, d_d, abs_o, abs_d), float64 (N,4): d_o = sum_s dp, d_d = sum_s z dp, component 3
    zero; abs_*: the sums of the terms' magnitudes (the scale a summation error is measured against)."""
    dp, z = np.asarray(d_points, np.float64), np.asarray(z, np.float64)
    pad = lambda a: np.concatenate([a, np.zeros((a.shape[0], 1))], -1)                              # noqa: E731
    zdp = z[..., None] * dp
    return pad(dp.sum(1)), pad(zdp.sum(1)), pad(np.abs(dp).sum(1)), pad(np.abs(zdp).sum(1))


def _render_rays(p, o, d, d_view, z, n_xyz, n_dir, n_angles, alpha, fp16_loss_scale=None):
    """T._render_rays with the direction of the sample points (d) and of the view-direction input (d_view) as two arguments;
    the same statements otherwise (tests/test_ray_gradients_host.py holds it to T._render_rays bit for bit)."""
    n, s = z.shape
    pts = (o[:, None, :3] + d[:, None, :3] * z[..., None]).reshape(-1, 3)
    comps = [0, 1, 2] if n_angles == 2 else [0, 2]
    view = d_view[:, comps][:, None, :].expand(n, s, len(comps)).reshape(-1, len(comps))
    dir_enc = None if n_angles == 0 else T._pe(view, n_dir, False)
    if fp16_loss_scale is not None:
        raw = T._mlp16(p, T._pe(pts, n_xyz, True), dir_enc, alpha, float(fp16_loss_scale)).reshape(n, s, 4)
    else:
        raw = T._mlp(p, T._pe(pts, n_xyz, True), dir_enc, alpha).reshape(n, s, 4)
    sigma = torch.relu(raw[..., 3])
    c = torch.sigmoid(raw[..., :3])
    delta = torch.cat([z[:, 1:] - z[:, :-1], torch.full((n, 1), 1e9, dtype=z.dtype)], -1)
    a = 1.0 - torch.exp(-sigma * delta)
    t = torch.cumprod(torch.cat([torch.ones((n, 1), dtype=z.dtype), 1.0 - a[:, :-1]], -1), -1)
    w = a * t
    return (w[..., None] * c).sum(1), w


def forward(pc, pf, o, d, near, far, u_c, u_f, n_xyz=5, n_dir=4, n_angles=2, alpha=0.05, sampler_grad=True, view_term=True,
            dtype=torch.float64, fp16_loss_scale=None):
    """R.render_outputs_forward on ray TENSORS o, d (N,4): -> (rgb, depth, weights, z) of the last pass, graph attached."""
    dv = d if view_term else d.detach()
    z = torch.tensor(O.get_z_values(near, far, np.asarray(u_c, np.float32)), dtype=dtype)
    rgb, w = _render_rays(pc, o, d, dv, z, n_xyz, n_dir, n_angles, alpha, fp16_loss_scale)
    if pf is not None:
        z_f = T._sample_pdf(w if sampler_grad else w.detach(), z, torch.tensor(np.asarray(u_f), dtype=dtype))
        z = torch.sort(torch.cat([z_f, z], -1), -1).values
        rgb, w = _render_rays(pf, o, d, dv, z, n_xyz, n_dir, n_angles, alpha, fp16_loss_scale)
    return rgb, (w * z).sum(-1), w, z


def ray_gradient_sets(blob_c, blob_f, rays_o, rays_d, near, far, u_c, u_f, sets, dtype=torch.float64, view_term=True, **kw):
    """Ray gradients for several cotangent sets on one forward graph.  sets: {name: dict of d_rgb / d_depth / d_weights /
    d_z}; keywords as R.render_outputs_gradients (n_pos_enc_xyz, n_pos_enc_dir, n_angles, alpha, sampler_grad,
    fp16_loss_scale).  -> dict(rgb, depth, weights, z, grads={name: (d_o, d_d)}), numpy; gradients (N,4), component 3 zero
    (the graph reads components 0..2 only)."""
    shape_kw = {k: kw[k] for k in ("n_pos_enc_xyz", "n_pos_enc_dir", "n_angles") if k in kw}
    pc = [t.detach() for t in T.blob_to_params(blob_c, dtype, **shape_kw)]
    pf = [t.detach() for t in T.blob_to_params(blob_f, dtype, **shape_kw)] if blob_f is not None else None
    o = torch.tensor(np.asarray(rays_o), dtype=dtype, requires_grad=True)
    d = torch.tensor(np.asarray(rays_d), dtype=dtype, requires_grad=True)
    outs = forward(pc, pf, o, d, near, far, u_c, u_f, kw.get("n_pos_enc_xyz", 5), kw.get("n_pos_enc_dir", 4),
                   kw.get("n_angles", 2), kw.get("alpha", 0.05), kw.get("sampler_grad", True), view_term, dtype,
                   kw.get("fp16_loss_scale"))
    grads = {}
    for name, cot in sets.items():
        loss = R._loss(outs, [cot.get(k) for k in ("d_rgb", "d_depth", "d_weights", "d_z")], dtype)
        if loss.requires_grad:
            gs = torch.autograd.grad(loss, (o, d), retain_graph=True, allow_unused=True)
        else:
            gs = (None, None)
        grads[name] = tuple((g if g is not None else torch.zeros_like(o)).numpy().copy() for g in gs)
    rgb, depth, w, z = (t.detach().numpy() for t in outs)
    return dict(rgb=rgb, depth=depth, weights=w, z=z, grads=grads)


def ray_gradients(blob_c, blob_f, rays_o, rays_d, near, far, u_c, u_f, d_rgb=None, d_depth=None, d_weights=None, d_z=None, **kw):
    """One cotangent set -> (d_o, d_d)."""
    cot = {k: v for k, v in dict(d_rgb=d_rgb, d_depth=d_depth, d_weights=d_weights, d_z=d_z).items() if v is not None}
    return ray_gradient_sets(blob_c, blob_f, rays_o, rays_d, near, far, u_c, u_f, {"one": cot}, **kw)["grads"]["one"]
