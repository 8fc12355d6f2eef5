"""torch.autograd bridge over the differentiable render outputs (include/nerf_mi355.h: nerf_train_render_forward_outputs /
nerf_train_render_backward_outputs): a training loss on the colour, the depth, the compositing weights or the sample depths of
``NeRF.render`` is one Python function of torch tensors.

    out = render_with_grad(ctx, rays_orig, rays_dirs, n_c, n_f)           # {"rgb", "depth", "weights", "z"}
    loss = ((out["depth"] - depth_target) ** 2).mean()                    # any torch expression of them
    loss.backward()                                                       # -> the context's gradient blobs
    ctx.train_apply()                                                     # Adam

The network weights live in the library, not in torch: the gradients of ``loss`` with respect to them land in the context's
gradient blobs (``ctx.train_get_gradients``), ready for ``ctx.train_apply()``.  The autograd node hangs on a scalar anchor
tensor that requires grad and receives a zero.  ``d_z`` and the depth's own dependence on z reach the networks only with a
fine pass under ``sampler_gradient`` (through the n_f new depths; the coarse depths are data).  Under mixed_float16 do NOT
scale the loss: the library multiplies the cotangents by its loss scale on the device and leaves unscaled gradients.
"""
from __future__ import annotations

from typing import Dict

OUTPUTS = ("rgb", "depth", "weights", "z")
_function = None


def _render_function():
    """The autograd node, built on first use (the package itself imports without torch)."""
    global _function
    if _function is not None:
        return _function
    import torch

    class _RenderWithGrad(torch.autograd.Function):
        @staticmethod
        def forward(fn, anchor, ctx, slot, accumulate, rays_orig, rays_dirs, n_c, n_f, u_coarse, u_fine, seed, ray_base):
            out = ctx.train_render_forward_outputs(slot, rays_orig, rays_dirs, n_c, n_f, u_coarse, u_fine, seed, ray_base,
                                                   outputs=OUTPUTS)
            if not all(isinstance(out[k], torch.Tensor) for k in OUTPUTS):
                raise TypeError("render_with_grad needs torch device tensors for rays_orig and rays_dirs")
            fn.set_materialize_grads(False)      # an output the loss did not use arrives as None, not as a zero tensor
            fn.call = (ctx, slot, accumulate)
            fn.anchor_like = anchor.detach()
            return tuple(out[k] for k in OUTPUTS)

        @staticmethod
        def backward(fn, d_rgb, d_depth, d_weights, d_z):
            ctx, slot, accumulate = fn.call
            grads = [None if g is None else g.detach().contiguous() for g in (d_rgb, d_depth, d_weights, d_z)]
            # consumes the slot: a second backward through the same graph fails with the library's "slot holds no forward pass"
            want_o, want_d = fn.needs_input_grad[4], fn.needs_input_grad[5]
            if not (want_o or want_d):
                ctx.train_render_backward_outputs(slot, *grads, accumulate=accumulate, want_blobs=False)
                return (torch.zeros_like(fn.anchor_like),) + (None,) * 11
            # rays that require grad: the library's ray gradients (its error if ctx.train_set_ray_gradients is off)
            _, _, g_o, g_d = ctx.train_render_backward_outputs(slot, *grads, accumulate=accumulate, want_blobs=False, want_rays=True)
            return (torch.zeros_like(fn.anchor_like), None, None, None, g_o if want_o else None, g_d if want_d else None) + \
                (None,) * 6

    _function = _RenderWithGrad
    return _function


def render_with_grad(ctx, rays_orig, rays_dirs, n_c, n_f, *, slot: int = 0, seed: int = 0, ray_base: int = 0,
                     accumulate: bool = False, u_coarse=None, u_fine=None) -> Dict[str, "torch.Tensor"]:
    """``NeRF.render`` on ``rays_orig``, ``rays_dirs`` (N,4; torch device tensors) under autograd: -> {"rgb" (N,3), "depth"
    (N,), "weights" (N,S), "z" (N,S)} of the last pass (S = n_c + n_f with a fine pass, else n_c), attached to one autograd
    node.  The forward keeps its activations in ``slot`` of ``ctx`` (a running trainer: ``ctx.train_begin``); ``backward()``
    of anything computed from the outputs makes the incoming cotangents contiguous, passes None for the outputs the loss did
    not use and calls ``ctx.train_render_backward_outputs(slot, ..., accumulate=accumulate)``: the gradients are stored in
    (or, ``accumulate``, added to) the context's blobs.  The backward consumes the slot, and so does an optimizer step: a
    second backward through the same graph (``retain_graph=True``) fails with the library's "slot holds no forward pass"
    message.  Under mixed_float16 the loss must not be scaled by the caller."""
    import torch
    like = rays_orig if isinstance(rays_orig, torch.Tensor) else None
    anchor = torch.zeros((), dtype=torch.float32, device=like.device if like is not None else None, requires_grad=True)
    out = _render_function().apply(anchor, ctx, int(slot), bool(accumulate), rays_orig, rays_dirs, int(n_c), int(n_f),
                                   u_coarse, u_fine, int(seed), int(ray_base))
    return dict(zip(OUTPUTS, out))
