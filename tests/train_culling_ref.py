"""Test-side restatement of the training graph under sample culling (include/nerf_mi355.h: nerf_ctx_set_train_sample_culling
has the rule), in torch on the CPU: oracle/train_oracle.py's train_gradients and render_gradients with

  * the coarse depths taken as DATA (under a grid the device narrows them: Context.get_z_values_for_rays with the same draws), and
  * the raw network output of every pass multiplied by a constant keep mask, which comes from tests/culling_ref.py::sample_keep
    evaluated on the restatement's own depths of that pass -- the coarse depths, the Sf new fine depths (train step) or the
    Sc + Sf merged depths (render gradients).

A culled sample therefore has raw output (0, 0, 0, 0), sends nothing back into the network or, through the network input, into
its depth; the compositing's own depth terms stay.  With an all-True mask the multiplication is by 1.0 and the functions are
the oracle's, operation for operation.  Imported by tests/test_train_culling_host.py and tests/test_gpu_train_culling.py."""
import math

import numpy as np
import torch

import culling_ref as K
from oracle.train_oracle import _mlp, _mlp16, _pe, _sample_pdf, blob_to_params


def keep_all(o, d, z):
    return np.ones(z.shape, bool)


def keep_none(o, d, z):
    return np.zeros(z.shape, bool)


def grid_keep(lo, hi, grid, dtype=K.F64):
    """-> keep(o, d, z): culling_ref.sample_keep under this box and grid (z is rounded to float32 on the way in)."""
    return lambda o, d, z: K.sample_keep(o, d, z, lo, hi, grid, dtype)


def face_margin(o, d, z, lo, hi, r):
    """How far the sample points o + d z (float64) stay from where the verdict can change, in cell edge lengths: for a point
    inside the box the distance to the nearest cell-face plane on any axis (box faces included); for a point outside it the
    distance by which it is outside (it is kept whatever the grid says).  -> the minimum over all samples."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    p = K.sample_points(o, d, np.asarray(z, np.float32), np.float64)
    t = (p - lo) / ((hi - lo) / r)
    outside = np.maximum(np.maximum(-t, t - r), 0.0).max(axis=-1)
    plane = np.abs(t - np.round(t)).min(axis=-1)
    return float(np.where(outside > 0, outside, plane).min())


def _render_rays(p, o, d, z, keep, n_xyz, n_dir, n_angles, alpha, fp16_loss_scale=None):
    """train_oracle._render_rays with raw * keep: -> (rgb (N,3), weights (N,S))."""
    n, s = z.shape
    pts = (o[:, None, :3] + d[:, None, :3] * z[..., None]).reshape(-1, 3)
    comps = [0, 1, 2] if n_angles == 2 else [0, 2]
    view = d[:, comps][:, None, :].expand(n, s, len(comps)).reshape(-1, len(comps))
    dir_enc = None if n_angles == 0 else _pe(view, n_dir, False)
    if fp16_loss_scale is not None:
        raw = _mlp16(p, _pe(pts, n_xyz, True), dir_enc, alpha, float(fp16_loss_scale)).reshape(n, s, 4)
    else:
        raw = _mlp(p, _pe(pts, n_xyz, True), dir_enc, alpha).reshape(n, s, 4)
    raw = raw * keep[..., None]
    sigma = torch.relu(raw[..., 3])
    c = torch.sigmoid(raw[..., :3])
    delta = torch.cat([z[:, 1:] - z[:, :-1], torch.full((n, 1), 1e9, dtype=z.dtype)], -1)
    a = 1.0 - torch.exp(-sigma * delta)
    T = torch.cumprod(torch.cat([torch.ones((n, 1), dtype=z.dtype), 1.0 - a[:, :-1]], -1), -1)
    w = a * T
    return (w[..., None] * c).sum(1), w


class _Graph:
    def __init__(self, blob_c, blob_f, rays_o, rays_d, keep_fn, dtype, kw):
        shape_kw = {k: kw[k] for k in ("n_pos_enc_xyz", "n_pos_enc_dir", "n_angles") if k in kw}
        self.net = (kw.get("n_pos_enc_xyz", 5), kw.get("n_pos_enc_dir", 4), kw.get("n_angles", 2), kw.get("alpha", 0.05))
        self.ls, self.sampler_grad, self.dtype = kw.get("fp16_loss_scale"), kw.get("sampler_grad", True), dtype
        self.pc = blob_to_params(blob_c, dtype, **shape_kw)
        self.pf = blob_to_params(blob_f, dtype, **shape_kw) if blob_f is not None else None
        self.o_np, self.d_np = np.asarray(rays_o, np.float32), np.asarray(rays_d, np.float32)
        self.o, self.d = torch.tensor(self.o_np, dtype=dtype), torch.tensor(self.d_np, dtype=dtype)
        self.keep_fn, self.keeps, self.depths = keep_fn, [], []

    def rays(self, p, z):
        """One pass on depths z: the mask is a constant taken from the depths' values."""
        zn = z.detach().numpy()
        keep = np.asarray(self.keep_fn(self.o_np, self.d_np, zn), bool)
        self.keeps.append(keep)
        self.depths.append(zn.astype(np.float64))
        return _render_rays(p, self.o, self.d, z, torch.tensor(keep.astype(np.float64), dtype=self.dtype), *self.net, self.ls)

    def grads(self, ps):
        return np.concatenate([(t.grad if t.grad is not None else torch.zeros_like(t)).numpy().ravel() for t in ps])


def train_gradients(blob_c, blob_f, rays_o, rays_d, target, z_coarse, u_f, keep_fn=keep_all, dtype=torch.float64, **kw):
    """train_oracle.train_gradients on the given coarse depths and under keep_fn(o, d, z) -> (N, S) bool
    -> dict(loss, psnr_coarse, psnr_fine, grad_coarse, grad_fine | None, z_fine, keeps [per pass], depths [per pass])."""
    g = _Graph(blob_c, blob_f, rays_o, rays_d, keep_fn, dtype, kw)
    tgt = torch.tensor(np.asarray(target), dtype=dtype)
    z = torch.tensor(np.asarray(z_coarse, np.float32), dtype=dtype)
    rgb_c, w_c = g.rays(g.pc, z)
    mse_c = ((rgb_c - tgt) ** 2).mean()
    loss, mse_f, z_f = mse_c, None, None
    if g.pf is not None:
        z_f = _sample_pdf(w_c if g.sampler_grad else w_c.detach(), z, torch.tensor(np.asarray(u_f), dtype=dtype))
        rgb_f, _ = g.rays(g.pf, z_f)
        mse_f = ((rgb_f - tgt) ** 2).mean()
        loss = loss + mse_f
    loss.backward()
    psnr = lambda m: float(-10.0 * math.log10(float(m.detach())))      # noqa: E731
    return dict(loss=float(loss.detach()), psnr_coarse=psnr(mse_c), psnr_fine=psnr(mse_f) if mse_f is not None else None,
                mse_coarse=float(mse_c.detach()), mse_fine=None if mse_f is None else float(mse_f.detach()),
                grad_coarse=g.grads(g.pc), grad_fine=g.grads(g.pf) if g.pf is not None else None,
                z_fine=None if z_f is None else z_f.detach().numpy(), keeps=g.keeps, depths=g.depths)


def render_gradients(blob_c, blob_f, rays_o, rays_d, d_rgb, z_coarse, u_f, keep_fn=keep_all, dtype=torch.float64, **kw):
    """train_oracle.render_gradients on the given coarse depths and under keep_fn: the fine pass runs, and is masked, on the
    Sc + Sf merged depths -> dict(rgb, grad_coarse, grad_fine | None, keeps, depths)."""
    g = _Graph(blob_c, blob_f, rays_o, rays_d, keep_fn, dtype, kw)
    z = torch.tensor(np.asarray(z_coarse, np.float32), dtype=dtype)
    rgb, w_c = g.rays(g.pc, z)
    if g.pf is not None:
        z_f = _sample_pdf(w_c if g.sampler_grad else w_c.detach(), z, torch.tensor(np.asarray(u_f), dtype=dtype))
        z_m = torch.sort(torch.cat([z_f, z], -1), -1).values
        rgb, _ = g.rays(g.pf, z_m)
    (rgb * torch.tensor(np.asarray(d_rgb), dtype=dtype)).sum().backward()
    return dict(rgb=rgb.detach().numpy(), grad_coarse=g.grads(g.pc), grad_fine=g.grads(g.pf) if g.pf is not None else None,
                keeps=g.keeps, depths=g.depths)
