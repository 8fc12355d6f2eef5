"""References for the distortion loss on the compositing weights -- TEST INFRASTRUCTURE ONLY.

For a ray with sorted depths z_0..z_{S-1} and weights w_i, with t_i = (z_i - near) / (far - near), t_S = 1, sample i owning
[t_i, t_{i+1}] (midpoint m_i, length d_i):

    L_ray = sum_i sum_j w_i w_j |m_i - m_j|  +  (1/3) sum_i w_i^2 d_i

    pairwise(w, z, near, far)           the definition itself, torch (float64 by default), differentiable: S^2 work
    pairwise_grads(w, z, near, far)     -> L_ray (N,), dL/dw (N,S), dL/dz (N,S) by float64 autograd of it
    restated(w, z, near, far, dtype)    the prefix-sum restatement the kernel evaluates, numpy at `dtype`
    has_ties(z, near, far)              whether two midpoints of a ray coincide (autograd's sign(0) = 0 differs there)
    train_gradients(...)                oracle.train_oracle.train_forward's graph with the two regulariser terms
"""
import math

import numpy as np
import torch

from oracle import nerf_oracle as O
from oracle.train_oracle import _render_rays, _sample_pdf, blob_to_params


def _intervals(z, near, far):
    """(m, d) of every sample; z: torch (N, S)."""
    t = (z - near) / (far - near)
    t1 = torch.cat([t[:, 1:], torch.ones((t.shape[0], 1), dtype=t.dtype)], -1)
    return (t + t1) / 2, t1 - t


def pairwise(w, z, near, far):
    """L_ray (N,) by the double sum; w, z: torch (N, S) of one dtype."""
    m, d = _intervals(z, near, far)
    pair = (w[:, :, None] * w[:, None, :] * (m[:, :, None] - m[:, None, :]).abs()).sum((1, 2))
    return pair + (w * w * d).sum(-1) / 3


def pairwise_grads(w, z, near, far):
    """float64 autograd of the definition -> (L_ray, dL/dw, dL/dz) as float64 numpy arrays."""
    wt = torch.tensor(np.asarray(w, np.float64), requires_grad=True)
    zt = torch.tensor(np.asarray(z, np.float64), requires_grad=True)
    loss = pairwise(wt, zt, float(near), float(far))
    loss.sum().backward()
    return loss.detach().numpy(), wt.grad.numpy(), zt.grad.numpy()


def has_ties(z, near, far):
    m, _ = _intervals(torch.tensor(np.asarray(z, np.float64)), float(near), float(far))
    return bool((m[:, 1:] <= m[:, :-1]).any())


def restated(w, z, near, far, dtype=np.float64):
    """The O(S) form with inclusive prefix sums P, Q (W, Qt their totals), every operation in `dtype`:
        A_i     = (m_i P_{i-1} - Q_{i-1}) + ((Qt - Q_i) - m_i (W - P_i))
        L_ray   = sum_i w_i A_i + (1/3) sum_i w_i^2 d_i
        dL/dw_i = 2 A_i + (2/3) w_i d_i
        dL/dm_i = 2 w_i (P_{i-1} - (W - P_i)),  dL/dd_i = w_i^2 / 3
        dL/dt_i = dL/dm_i / 2 - dL/dd_i + dL/dm_{i-1} / 2 + dL/dd_{i-1},   dL/dz_i = dL/dt_i / (far - near)
    -> (L_ray (N,), dL/dw (N,S), dL/dz (N,S)) in `dtype`."""
    f = np.dtype(dtype).type
    w, z = np.asarray(w, dtype), np.asarray(z, dtype)
    near, rng = f(near), f(far) - f(near)
    n = w.shape[0]
    t = (z - near) / rng
    t1 = np.concatenate([t[:, 1:], np.ones((n, 1), dtype)], -1)
    m, d = (t + t1) * f(0.5), t1 - t
    P, Q = np.cumsum(w, -1, dtype=dtype), np.cumsum(w * m, -1, dtype=dtype)
    zero = np.zeros((n, 1), dtype)
    Pe, Qe = np.concatenate([zero, P[:, :-1]], -1), np.concatenate([zero, Q[:, :-1]], -1)
    W, Qt = P[:, -1:], Q[:, -1:]
    A = (m * Pe - Qe) + ((Qt - Q) - m * (W - P))
    loss = (w * A + w * w * d / f(3)).sum(-1, dtype=dtype)
    dw = f(2) * A + f(2) * w * d / f(3)
    dm, dd = f(2) * w * (Pe - (W - P)), w * w / f(3)
    dm_prev, dd_prev = np.concatenate([zero, dm[:, :-1]], -1), np.concatenate([zero, dd[:, :-1]], -1)
    dt = f(0.5) * dm - dd + f(0.5) * dm_prev + dd_prev
    return loss, dw, dt / rng


def operator_inputs(n, s, near, far, seed=0):
    """Weights as compositing makes them (alpha * exclusive cumprod of 1 - alpha, some alphas exactly 0, ray 1 all zeros) and
    sorted depths without ties, float32."""
    rng = np.random.default_rng(seed)
    alpha = rng.random((n, s)) * (2.0 / max(s, 2) ** 0.5)
    alpha = np.minimum(alpha, 0.95)
    alpha[rng.random((n, s)) < 0.2] = 0.0
    if n > 1:
        alpha[1] = 0.0
    T = np.cumprod(np.concatenate([np.ones((n, 1)), 1.0 - alpha[:, :-1]], -1), -1)
    w = (alpha * T).astype(np.float32)
    # strictly increasing depths inside (near, far): jittered strata
    z = near + (far - near) * (np.arange(s)[None, :] + 0.1 + 0.8 * rng.random((n, s))) / s
    z = z.astype(np.float32)
    assert (np.diff(z, axis=-1) > 0).all() and not has_ties(z, near, far)
    return w, z


def train_gradients(blob_c, blob_f, rays_o, rays_d, target, near, far, u_c, u_f, loss_w=(1.0, 1.0), lam=(0.0, 0.0),
                    sampler_grad=True, alpha=0.05, dz_term=True, dtype=torch.float64, fp16_loss_scale=None):
    """oracle.train_oracle.train_forward's graph with the regulariser:
        objective = loss_w[0] MSE_c + loss_w[1] MSE_f + lam[0] L(coarse pass) + lam[1] L(fine pass),  L = mean of L_ray.
    The coarse depths are data; the fine depths come out of the sampler, differentiable in the coarse weights when
    sampler_grad.  dz_term = False cuts dL/dz of the fine pass's regulariser (what a trainer that forgot it would compute).
    fp16_loss_scale: the networks under the library's mixed_float16 arithmetic (oracle.train_oracle._mlp16).
    -> dict(loss (the weighted MSE sum), dist_coarse, dist_fine (the unweighted L), grad_coarse, grad_fine)."""
    pc, pf = blob_to_params(blob_c, dtype), blob_to_params(blob_f, dtype)
    T = lambda a: torch.tensor(np.asarray(a), dtype=dtype)                                     # noqa: E731
    o, d, tgt = T(rays_o), T(rays_d), T(target)
    z = T(O.get_z_values(near, far, np.asarray(u_c, np.float32)))
    near, far = float(near), float(far)
    rgb_c, w_c = _render_rays(pc, o, d, z, 5, 4, 2, alpha, fp16_loss_scale)
    mse_c = ((rgb_c - tgt) ** 2).mean()
    dist_c = pairwise(w_c, z, near, far).mean()
    z_f = _sample_pdf(w_c if sampler_grad else w_c.detach(), z, T(u_f))
    rgb_f, w_f = _render_rays(pf, o, d, z_f, 5, 4, 2, alpha, fp16_loss_scale)
    mse_f = ((rgb_f - tgt) ** 2).mean()
    dist_f = pairwise(w_f, z_f if dz_term else z_f.detach(), near, far).mean()
    mse = loss_w[0] * mse_c + loss_w[1] * mse_f
    (mse + lam[0] * dist_c + lam[1] * dist_f).backward()
    g = lambda ps: np.concatenate([(t.grad if t.grad is not None else torch.zeros_like(t)).numpy().ravel()   # noqa: E731
                                   for t in ps])
    psnr = lambda v: float(-10.0 * math.log10(float(v.detach())))                              # noqa: E731
    return dict(loss=float(mse.detach()), psnr_coarse=psnr(mse_c), psnr_fine=psnr(mse_f), dist_coarse=float(dist_c.detach()),
                dist_fine=float(dist_f.detach()), grad_coarse=g(pc), grad_fine=g(pf))
