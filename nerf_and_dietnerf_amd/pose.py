"""Rays from a camera pose as a differentiable torch function -- the caller's half of pose refinement.

    pose = torch.nn.Parameter(c2w)                                         # (4,4) camera-to-world
    o, d = rays_from_pose(pose, fov, H, W, pixel_index)                    # differentiable in `pose`
    out = render_with_grad(ctx, o, d, n_c, n_f)                            # ctx.train_set_ray_gradients(True)
    ((out["rgb"] - target) ** 2).mean().backward()                         # -> pose.grad (and the context's weight blobs)

``rays_from_pose`` restates ``nerf_get_rays_directions`` (src/UtilsCV.py:467-499: pixel centres, xy meshgrid, the same tangent
for both axes, the camera looking down -z) and the origin broadcast of ``render_image`` (every ray starts at c2w[:, 3]) in
torch operations, so autograd carries d_rays_orig / d_rays_dirs back into the pose.  torch is imported on first use: the
package itself imports without it.
"""
from __future__ import annotations

import math


def rays_from_pose(c2w, fov: float, H: int, W: int, pixel_index=None):
    """``c2w`` (4,4) torch tensor, ``fov`` the field of view in radians, ``H`` x ``W`` pixels -> (rays_orig, rays_dirs), each
    (H*W, 4) in row-major pixel order, or (len(pixel_index), 4) for ``pixel_index`` (flat indices y * W + x, a tensor or a
    sequence).  rays_dirs[i] = c2w @ (x_c, y_c, -1, 0), un-normalised, as the library's ray generator forms it; rays_orig[i] =
    c2w[:, 3].  Differentiable in ``c2w``; the tangent is taken of float32(fov / 2) in double and rounded once."""
    import torch
    if tuple(c2w.shape) != (4, 4):
        raise ValueError("c2w must be (4,4)")
    dt, dev = c2w.dtype, c2w.device
    if pixel_index is None:
        idx = torch.arange(H * W, device=dev)
    else:
        idx = torch.as_tensor(pixel_index, device=dev).reshape(-1).long()
    xr = (idx % W).to(dt) + 0.5
    yr = torch.div(idx, W, rounding_mode="floor").to(dt) + 0.5
    x_ss = 2.0 * (xr / W) - 1.0
    y_ss = 1.0 - 2.0 * (yr / H)
    tan_half = float(torch.tensor(math.tan(float(torch.tensor(fov / 2, dtype=torch.float32))), dtype=torch.float32))
    xc, yc = x_ss * tan_half, y_ss * tan_half
    # ((c0 x + c1 y) + c2 z) + c3 0 with z = -1: the generator's order of operations
    dirs = (c2w[:, 0][None, :] * xc[:, None] + c2w[:, 1][None, :] * yc[:, None]) - c2w[:, 2][None, :]
    orig = c2w[:, 3][None, :].expand(idx.shape[0], 4)
    return orig, dirs
