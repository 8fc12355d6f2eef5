"""Host-side mirror of the reference's render call surface, over the C ABI of libnerf_mi355.so.

Same names, argument meaning and error behaviour as the reference (paths under /root/reference):
    NeRF.render / render_image / render_rays / call          src/NeRF.py:96-246
    render_rays, ray_marching, model_predict,
    positional_encoding_for_xyz/_for_views,
    split_to_batches, get_size_of_splits                     src/UtilsNeuralRadianceField.py:17-234
    get_rays_directions, get_z_values,
    get_z_vals_from_prob_dist_func                           src/UtilsCV.py:467-581

Arrays may be numpy (host: the library stages them) or torch CUDA tensors (device: used in place on
torch's current stream); outputs come back in the same kind.  The two random draws the reference
takes from tf.random.uniform are explicit (``u_coarse``/``u_fine``/``uniform_values``) or come
from the on-device Philox generator keyed by ``seed`` and the global ray index.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import (NerfTrainConfig, NERF_MEM_DEVICE, NERF_MEM_HOST, NERF_NET_COARSE, NERF_NET_FINE, NERF_PRECISION_F16X3,
                   NERF_PRECISION_FP32, NerfConfig, NerfOutputs)
from .sh import SH_MAX_DIRS, check_sh_degree, sh_basis_count, sh_degree_of, sh_quadrature, sh_texel_floats

# configuration key names (src/ConfigurationKeys.py:64-111)
N_RENDER_SAMPLES_FINE = "n_render_samples_fine"
N_RENDER_SAMPLES_COARSE = "n_render_samples_coarse"
N_POS_ENC_DIM_XYZ = "n_pos_enc_dim_xyz"
N_POS_ENC_VIEW_DIR = "n_pos_enc_view_dir"
N_ANGLES_FOR_MODEL = "n_angles_for_model"
LEAKY_RELU_ALPHA = "leaky_relu_alpha"
HIDDEN_LAYER_DIM = "hidden_layer_dim"
LAST_HIDDEN_LAYER_DIM = "last_hidden_layer_dim"
N_RAYS_IN_BATCH_RENDER = "n_rays_in_batch_render"
N_RAYS_IN_BATCH_TRAIN = "n_rays_in_batch_train"
# render_config keys the reference does not have: forward-facing scenes ("Ray and sampling space")
LINDISP = "lindisp"                  # bool, default False: coarse depths uniform in disparity
USE_NDC = "use_ndc"                  # bool, default False: rays in normalised device coordinates
NDC_NEAR_PLANE = "ndc_near_plane"    # float, default 1.0: distance of the NDC near plane (with use_ndc)
SCENE_BOX = "scene_box"              # [[x, y, z], [x, y, z]] (lo, hi), default absent: per-ray depth range from a scene box
OCCUPANCY_GRID = "occupancy_grid"    # dict of the keys below, default absent: sample each ray where the network has density
GRID_RESOLUTION, GRID_SIGMA_THRESHOLD, GRID_SAMPLES_PER_CELL = "resolution", "sigma_threshold", "samples_per_cell"
GRID_DILATE, GRID_UPDATE_EVERY, GRID_WARMUP_EPOCHS = "dilate", "update_every", "warmup_epochs"
GRID_CULL_SAMPLES = "cull_samples"    # bool, default False: samples in empty cells skip the network (Context.set_sample_culling)
GRID_CULL_TRAIN_SAMPLES = "cull_train_samples"    # bool, default False: the same in the trainer (Context.set_train_sample_culling)
_GRID_KEYS = (GRID_RESOLUTION, GRID_SIGMA_THRESHOLD, GRID_SAMPLES_PER_CELL, GRID_DILATE, GRID_UPDATE_EVERY, GRID_WARMUP_EPOCHS,
              GRID_CULL_SAMPLES, GRID_CULL_TRAIN_SAMPLES)
GRID_NEEDS_BOX = "an occupancy grid needs a scene box"
DISTORTION_LOSS = "distortion_loss"  # number, or [coarse, fine], default absent: weights of the distortion regulariser in training
ENCODING_WINDOW = "encoding_window"  # dict of the keys below, default absent: coarse-to-fine positional encoding over the fit epochs
WINDOW_KIND, WINDOW_START, WINDOW_END, WINDOW_EPOCHS, WINDOW_DIRS = "kind", "start", "end", "epochs", "dirs"
_WINDOW_KEYS = (WINDOW_KIND, WINDOW_START, WINDOW_END, WINDOW_EPOCHS, WINDOW_DIRS)
_WINDOW_KINDS = ("cosine", "linear")

N_COORDINATES = 3
N_COLOR_CHANNELS = 3

# "auto": render in f16x3 (fp32-class results at 3x the exact-fp32 rate), watch the library's non-finite counter, and fall
# back to exact fp32 for a weight set whose activations leave the fp16 range (Context._auto_call)
_PRECISIONS = {"fp32": NERF_PRECISION_FP32, "f16x3": NERF_PRECISION_F16X3, "f16": _lib.NERF_PRECISION_F16,
               "bf16x3": _lib.NERF_PRECISION_BF16X3, "auto": NERF_PRECISION_F16X3}
_SAMPLINGS = {"linear": _lib.NERF_SAMPLING_LINEAR, "lindisp": _lib.NERF_SAMPLING_LINDISP}
_RAY_SPACES = {"world": _lib.NERF_RAYS_WORLD, "ndc": _lib.NERF_RAYS_NDC}


# --------------------------------------------------------------------------------------------
# array plumbing: numpy (host) or torch.cuda (device)
# --------------------------------------------------------------------------------------------
def check_grid_resolution(resolution) -> int:
    """The library's rule for R (a multiple of 4 in [4, 256]), checked before any device call."""
    r = int(resolution)
    if r != resolution or r < 4 or r > 256 or r % 4:
        raise ValueError(f"occupancy grid resolution must be a multiple of 4 in [4, 256] (got {resolution!r})")
    return r


def check_distortion_loss(value) -> Tuple[float, float]:
    """render_config["distortion_loss"] -> (coarse, fine): one number for both passes, or [coarse, fine]; finite, >= 0."""
    def number(v):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError(f"{DISTORTION_LOSS} must be a number or [coarse, fine] (got {value!r})")
        v = float(v)
        if not (np.isfinite(v) and v >= 0):
            raise ValueError(f"{DISTORTION_LOSS} weights must be finite and >= 0 (got {value!r})")
        return v
    if isinstance(value, (list, tuple, np.ndarray)):
        if len(value) != 2:
            raise ValueError(f"{DISTORTION_LOSS} must be a number or [coarse, fine] (got {value!r})")
        return number(value[0]), number(value[1])
    v = number(value)
    return v, v


def encoding_window(alpha, n_octaves, kind="cosine") -> np.ndarray:
    """The coarse-to-fine window at progress ``alpha`` in [0, n_octaves]: the weight of octave k, float32 (n_octaves,).
    "cosine" (BARF): 0 for alpha < k, (1 - cos((alpha - k) pi)) / 2 for 0 <= alpha - k < 1, 1 above.  "linear" (FreeNeRF's
    ramp): clip(alpha - k, 0, 1).  alpha = 0 masks every octave, alpha >= n_octaves none."""
    if kind not in _WINDOW_KINDS:
        raise ValueError(f"encoding window kind must be one of {_WINDOW_KINDS} (got {kind!r})")
    n = int(n_octaves)
    if n != n_octaves or n < 1:
        raise ValueError(f"encoding window: n_octaves must be a positive integer (got {n_octaves!r})")
    alpha = float(alpha)
    if not np.isfinite(alpha):
        raise ValueError(f"encoding window: alpha must be finite (got {alpha!r})")
    t = np.clip(alpha - np.arange(n, dtype=np.float64), 0.0, 1.0)
    w = t if kind == "linear" else (1.0 - np.cos(t * np.pi)) / 2.0
    return w.astype(np.float32)


def check_encoding_window(value, n_octaves) -> dict:
    """render_config["encoding_window"] -> the dict with defaults filled in: kind "cosine", start 0, end n_octaves, epochs
    (required, a positive integer), dirs False.  An unknown key, kind or a value out of range fails."""
    if not isinstance(value, dict):
        raise ValueError(f"{ENCODING_WINDOW} must be a dict with keys from {_WINDOW_KEYS} (got {value!r})")
    unknown = set(value) - set(_WINDOW_KEYS)
    if unknown:
        raise ValueError(f"unknown {ENCODING_WINDOW} keys {sorted(unknown)}: expected {_WINDOW_KEYS}")
    if WINDOW_EPOCHS not in value:
        raise ValueError(f"{ENCODING_WINDOW} needs \"{WINDOW_EPOCHS}\": the fit epochs over which the window opens")
    kind = value.get(WINDOW_KIND, "cosine")
    if kind not in _WINDOW_KINDS:
        raise ValueError(f"{ENCODING_WINDOW} kind must be one of {_WINDOW_KINDS} (got {kind!r})")
    epochs = value[WINDOW_EPOCHS]
    if isinstance(epochs, bool) or int(epochs) != epochs or epochs < 1:
        raise ValueError(f"{ENCODING_WINDOW} {WINDOW_EPOCHS} must be a positive integer (got {epochs!r})")
    start, end = float(value.get(WINDOW_START, 0.0)), float(value.get(WINDOW_END, n_octaves))
    if not (np.isfinite(start) and np.isfinite(end) and 0.0 <= start <= end):
        raise ValueError(f"{ENCODING_WINDOW} needs finite 0 <= start <= end (got start {start!r}, end {end!r})")
    return {WINDOW_KIND: kind, WINDOW_START: start, WINDOW_END: end, WINDOW_EPOCHS: int(epochs),
            WINDOW_DIRS: bool(value.get(WINDOW_DIRS, False))}


def encoding_window_alpha(cfg, epoch) -> float:
    """alpha_xyz at the start of fit epoch ``epoch`` (0-based) under a checked config: start + (end - start) min(e / E, 1)."""
    return cfg[WINDOW_START] + (cfg[WINDOW_END] - cfg[WINDOW_START]) * min(epoch / cfg[WINDOW_EPOCHS], 1.0)


def pack_occupancy_grid(grid) -> np.ndarray:
    """(R, R, R) bool array indexed [ix, iy, iz] -> R^3 / 32 little-endian uint32 words, cell (ix, iy, iz) = bit
    ix + R (iy + R iz)."""
    g = np.asarray(grid)
    if g.ndim != 3 or g.shape[0] != g.shape[1] or g.shape[0] != g.shape[2]:
        raise ValueError(f"an occupancy grid is an (R, R, R) array, got shape {g.shape}")
    check_grid_resolution(g.shape[0])
    flat = np.ascontiguousarray(g.astype(bool).transpose(2, 1, 0)).ravel()          # ix runs fastest
    return np.packbits(flat, bitorder="little").view("<u4").astype(np.uint32)


def unpack_occupancy_grid(words, resolution=None) -> np.ndarray:
    """The inverse of pack_occupancy_grid; ``resolution`` defaults to the R with R^3 = 32 * len(words)."""
    w = np.ascontiguousarray(np.asarray(words).ravel(), dtype="<u4")
    r = int(round((32 * w.size) ** (1.0 / 3.0))) if resolution is None else int(resolution)
    check_grid_resolution(r)
    if r ** 3 != 32 * w.size:
        raise ValueError(f"{w.size} words are no R^3 / 32 for R = {r}")
    return np.unpackbits(w.view(np.uint8), bitorder="little").astype(bool).reshape(r, r, r).transpose(2, 1, 0).copy()


def _is_torch(x) -> bool:
    return hasattr(x, "data_ptr") and hasattr(x, "is_cuda")


def _host_floats(x, shape, name, exact=False) -> np.ndarray:
    """A small host argument (numpy array, list or torch tensor) as a contiguous float32 array of ``shape``.  It may come in any
    shape with that many components, unless ``exact`` asks for ``shape`` itself; shape None: any size, flattened."""
    a = np.ascontiguousarray(x.detach().cpu().numpy() if _is_torch(x) else x, dtype=np.float32)
    if shape is None:
        return a.ravel()
    if exact and a.shape != tuple(shape):
        raise ValueError(f"{name} must be ({','.join(map(str, shape))})")
    if a.size != int(np.prod(shape)):
        raise ValueError(f"{name} must have {int(np.prod(shape))} components, got {a.size}")
    return a.reshape(shape)


def _box_corners(lo, hi) -> Tuple[np.ndarray, np.ndarray]:
    lo_a, hi_a = _host_floats(lo, None, "lo"), _host_floats(hi, None, "hi")
    if lo_a.size != 3 or hi_a.size != 3:
        raise ValueError(f"box corners must have 3 components each, got {lo_a.size} and {hi_a.size}")
    return lo_a, hi_a


class _PinnedBlock:
    """One nerf_host_alloc allocation seen as a numpy array: ``np.asarray(block)`` makes an array whose ``base`` is this
    object, so the block lives exactly as long as the array or any view of it; then it returns to the pool."""

    def __init__(self, pool, ptr: int, cap: int, n_floats: int):
        self._pool, self.ptr, self.cap = pool, ptr, cap
        self.__array_interface__ = {"data": (ptr, False), "shape": (n_floats,), "typestr": "<f4", "version": 3}

    def __del__(self):
        try:
            self._pool._give_back(self.ptr, self.cap)
        except Exception:      # interpreter shutdown: the process is about to release everything anyway
            pass


class _PinnedPool:
    """Page-locked output buffers for host-memory calls (include/nerf_mi355.h: nerf_host_alloc).  The reference returns
    fresh tensors from every call (src/NeRF.py:239-246); so does this: a block is handed out again only after every numpy
    reference to its previous use is gone.  Pinning costs ~0.2 ms per MB, hence the reuse; at most ``keep_bytes`` of free
    blocks are kept.

    Page-locked memory cannot be swapped, so the pool is BOUNDED: live (handed-out) plus free blocks never exceed
    ``budget_bytes``.  A request that does not fit first releases free blocks; if it still does not fit -- a caller that keeps
    hundreds of frames alive -- or if nerf_host_alloc itself fails, ``take`` returns None and the caller falls back to an
    ordinary pageable ``np.empty`` (the C side accepts any host memory; only the copy/compute overlap is lost)."""
    MIN_BYTES = 256 << 10       # smaller outputs are ordinary numpy arrays
    GRAIN = 2 << 20             # blocks of 8 MiB and more are rounded up to this ...
    SMALL_GRAIN = 128 << 10     # ... smaller ones (an rgb frame: 786 KB at 256 x 256) to this

    def __init__(self, keep_bytes: int = 4 << 30, budget_bytes: int = 8 << 30):
        import threading
        self.free: List[Tuple[int, int]] = []        # (cap, ptr)
        self.keep_bytes, self.free_bytes = keep_bytes, 0
        self.budget_bytes, self.live_bytes = budget_bytes, 0
        self.fallbacks = 0                           # requests served from pageable memory instead
        # re-entrant: a garbage collection inside take() may run a dead block's __del__ -> _give_back on this same thread
        self.lock = threading.RLock()

    def _grain(self, nbytes: int) -> int:
        return self.GRAIN if nbytes >= (8 << 20) else self.SMALL_GRAIN

    def take(self, shape) -> Optional[np.ndarray]:
        n = int(np.prod(shape, dtype=np.int64))
        nbytes = 4 * n
        lib = _lib.load()
        release: List[int] = []
        with self.lock:
            best = None
            for i, (cap, _) in enumerate(self.free):
                if nbytes <= cap <= nbytes + nbytes // 4 + self._grain(nbytes) and (best is None or cap < self.free[best][0]):
                    best = i
            if best is not None:
                cap, ptr = self.free.pop(best)
                self.free_bytes -= cap
            else:
                g = self._grain(nbytes)
                cap, ptr = -(-nbytes // g) * g, None
                # make room: free blocks go first, then the request is refused
                while self.live_bytes + self.free_bytes + cap > self.budget_bytes and self.free:
                    fcap, fptr = self.free.pop()
                    self.free_bytes -= fcap
                    release.append(fptr)
                if self.live_bytes + self.free_bytes + cap > self.budget_bytes:
                    cap = 0
            if cap:
                self.live_bytes += cap
        for fptr in release:
            lib.nerf_host_free(C.c_void_p(fptr))
        if not cap:
            self.fallbacks += 1
            return None
        if ptr is None:
            out = C.c_void_p()
            if lib.nerf_host_alloc(cap, C.byref(out)) != 0 or not out.value:      # the host cannot pin more: pageable
                with self.lock:
                    self.live_bytes -= cap
                    self.fallbacks += 1
                return None
            ptr = out.value
        return np.asarray(_PinnedBlock(self, ptr, cap, n)).reshape(tuple(shape))

    def _give_back(self, ptr: int, cap: int) -> None:
        with self.lock:
            self.live_bytes -= cap
            if self.free_bytes + cap <= self.keep_bytes:
                self.free.append((cap, ptr))
                self.free_bytes += cap
                return
        _lib.load().nerf_host_free(C.c_void_p(ptr))

    def trim(self) -> None:
        """Release every free block."""
        with self.lock:
            blocks, self.free, self.free_bytes = self.free, [], 0
        for _, ptr in blocks:
            _lib.load().nerf_host_free(C.c_void_p(ptr))


_pinned = _PinnedPool()


class _Arrays:
    """Decides host/device for one call, keeps converted inputs alive, allocates outputs."""

    def __init__(self, *probe):
        self.torch = None
        self.keep = []
        dev = [p for p in probe if p is not None and _is_torch(p) and p.is_cuda]
        if dev:
            import torch
            self.torch = torch
            self.device = dev[0].device
        self.mem = NERF_MEM_DEVICE if self.torch else NERF_MEM_HOST

    def inp(self, x, shape=None) -> Optional[int]:
        if x is None:
            return None
        if self.torch:
            t = x if _is_torch(x) else self.torch.as_tensor(np.asarray(x, np.float32))
            t = t.to(device=self.device, dtype=self.torch.float32).contiguous()
            if shape is not None and tuple(t.shape) != tuple(shape):
                raise ValueError(f"expected shape {tuple(shape)}, got {tuple(t.shape)}")
            self.keep.append(t)
            return t.data_ptr()
        if _is_torch(x):
            x = x.detach().cpu().numpy()
        a = np.ascontiguousarray(np.asarray(x), dtype=np.float32)
        if shape is not None and tuple(a.shape) != tuple(shape):
            raise ValueError(f"expected shape {tuple(shape)}, got {tuple(a.shape)}")
        self.keep.append(a)
        return a.ctypes.data

    def out(self, shape, dtype=np.float32):
        if self.torch:
            t = self.torch.empty(tuple(shape), dtype=getattr(self.torch, np.dtype(dtype).name), device=self.device)
            self.keep.append(t)
            return t, t.data_ptr()
        nbytes = 4 * int(np.prod(shape, dtype=np.int64))
        a = _pinned.take(shape) if dtype is np.float32 and nbytes >= _PinnedPool.MIN_BYTES else None
        if a is None:                # small or non-float32 output, pinned budget exhausted or pinning failed: pageable memory
            a = np.empty(tuple(shape), dtype)
        self.keep.append(a)
        return a, a.ctypes.data


class Context:
    """One nerf_ctx: one GPU, one stream, both networks' weights, a scratch arena."""

    def __init__(self, *, n_pos_enc_xyz=5, n_pos_enc_dir=4, n_angles=2, hidden_dim=256, last_hidden_dim=128,
                 leaky_relu_alpha=0.05, near=2.0, far=6.0, precision="auto", device=0):
        """``precision``: "auto" (default: f16x3 with the fallback below -- to exact fp32, or to bf16x3 for a network with
        n_pos_enc_xyz 6..10, which has no exact-fp32 kernel), "fp32" (exact fp32 MFMA: the parity mode), "f16x3" (3-pass
        split-fp16 MFMA, fp32-class results while |activations| < 65504), "bf16x3" (3-pass split-bf16 MFMA: fp32-class
        results, 1e-4 RGB, with fp32's exponent range; render path only), "f16" (single-pass fp16: the numerics class of
        the reference's mixed_float16 policy)."""
        self.lib = _lib.load()
        if n_angles not in (0, 1, 2):
            raise Exception(f"{N_ANGLES_FOR_MODEL} should be 1 or 2.")   # src/UtilsCV.py:138
        self.n_angles = n_angles
        self.cfg = NerfConfig(n_pos_enc_xyz, n_pos_enc_dir, n_angles, hidden_dim, last_hidden_dim,
                              leaky_relu_alpha, near, far, _PRECISIONS[precision], device)
        h = C.c_void_p()
        _lib.check(self.lib.nerf_ctx_create(C.byref(self.cfg), C.byref(h)))
        self.h = h
        self.loaded = [False, False]
        self._stream = None
        self.comm_world = 0          # ranks of this ctx's in-library communicator (0 = none)
        self.precision = precision
        self._auto_fp32 = False      # "auto": this weight set overflowed fp16 once -> exact fp32 (n_pos_enc_xyz 6..10: bf16x3) until the weights change
        self._auto_unchecked = False  # "auto": device-resident calls since the last look at the counter
        self.auto_fallbacks = 0      # "auto": calls that were re-rendered in exact fp32
        self._slot_fine = {}         # train_render_forward slots that ran a fine pass
        self._slot_rays = {}         # ... and how many rays each holds
        self._train_ray_gradients = False   # train_set_ray_gradients
        self.sampling, self.ray_space, self.ndc_near_plane = "linear", "world", 1.0   # what nerf_ctx_create leaves
        self.scene_box = None        # ((lo), (hi)) of set_scene_box
        self.grid_resolution = 0     # R of the occupancy grid (0: none)
        self.sample_culling = False  # set_sample_culling
        self._train_sample_culling = False  # set_train_sample_culling

    def close(self):
        if getattr(self, "h", None):
            self.lib.nerf_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- weights ----
    def blob_size(self) -> int:
        return int(self.lib.nerf_blob_size(C.byref(self.cfg)))

    def load_weights(self, which: int, weights) -> None:
        """``weights``: flat fp32 blob, or the Keras ``model.get_weights()`` list (22 arrays,
        kernel(in,out) then bias, layers in creation order src/NeRF.py:319-337)."""
        if isinstance(weights, (list, tuple)):
            blob = np.concatenate([np.asarray(w, np.float32).ravel() for w in weights])
        else:
            blob = np.ascontiguousarray(np.asarray(weights, np.float32).ravel())
        _lib.check(self.lib.nerf_load_weights(self.h, which, blob.ctypes.data, blob.size))
        self.loaded[which] = True
        self._auto_new_weights()

    # ---- coarse-to-fine positional encoding (include/nerf_mi355.h: nerf_ctx_set_encoding_window has the rules) ----
    def set_encoding_window(self, xyz=None, dirs=None) -> None:
        """A weight in [0, 1] per octave of the xyz encoding (``xyz``: n_pos_enc_xyz values) and of the direction encoding
        (``dirs``: n_pos_enc_dir values; accepted and without effect when n_angles is 0); None = all ones, and all ones is
        "off".  Every network evaluation of the context then sees octave k's sin / cos features times its weight -- renders,
        model_predict, the lattice, the bake, every trainer pass -- while the pass-through component keeps weight 1.  The
        master weights are never scaled (get_weights, checkpoints and Adam's moments do not know of the window) and weight
        gradients are with respect to the master weights: a row with weight 0 gets gradient 0 and is not trained.  The window
        belongs to the context and survives load_weights, train_begin and train_end.  Setting it re-packs the loaded
        networks and a running trainer's on the context's stream without synchronising; it fails while a render slot holds
        a forward pass (run its backward first).  An occupancy grid is kept as baked.  Under data-parallel training every
        rank's context must be given the same window: nothing synchronises it."""
        def vec(name, v, n):
            if v is None:
                return None
            a = np.ascontiguousarray(np.asarray(v, np.float32).ravel())
            if a.size != n:
                raise ValueError(f"encoding window: {name} needs {n} values, one per octave (got {a.size})")
            return a
        wx = vec("xyz", xyz, int(self.cfg.n_pos_enc_xyz))
        wd = vec("dirs", dirs, int(self.cfg.n_pos_enc_dir))
        _lib.check(self.lib.nerf_ctx_set_encoding_window(self.h, None if wx is None else wx.ctypes.data,
                                                        None if wd is None else wd.ctypes.data))
        self._auto_new_weights()         # "auto": what the networks compute has changed, as with new weights

    def encoding_window(self):
        """(xyz, dirs) float32 arrays of the window in force, or None when it is off."""
        wx, wd = np.empty(int(self.cfg.n_pos_enc_xyz), np.float32), np.empty(int(self.cfg.n_pos_enc_dir), np.float32)
        active = C.c_int32()
        _lib.check(self.lib.nerf_ctx_get_encoding_window(self.h, wx.ctypes.data, wd.ctypes.data, C.byref(active)))
        return (wx, wd) if active.value else None

    def set_bounds(self, near: float, far: float) -> None:
        _lib.check(self.lib.nerf_ctx_set_bounds(self.h, near, far))
        self.cfg.near_boundary, self.cfg.far_boundary = near, far

    def set_sampling(self, mode: str) -> None:
        """"linear" (default: coarse depths stratified uniformly in depth, src/UtilsCV.py:565-581) or "lindisp" (uniformly in
        disparity 1/z; needs near > 0).  Every call that draws coarse depths follows it: get_z_values, render, render_image,
        the trainer."""
        if mode not in _SAMPLINGS:
            raise ValueError(f"unknown sampling mode {mode!r}: expected one of {sorted(_SAMPLINGS)}")
        # the library's own check (it repeats it wherever depths are drawn: the bounds may change later), made here first so
        # that a configuration error does not need a device call to show
        if mode == "lindisp" and not self.cfg.near_boundary > 0:
            raise RuntimeError("lindisp needs near_boundary > 0")
        _lib.check(self.lib.nerf_ctx_set_sampling(self.h, _SAMPLINGS[mode]))
        self.sampling = mode

    def set_ray_space(self, space: str, ndc_near_plane: float = 1.0) -> None:
        """"world" (default) or "ndc": render_image / render_image_sharded then pass the camera's rays through
        ``rays_to_ndc(..., fov, ndc_near_plane)`` before rendering; set the bounds to (0, 1) for it.  Calls that take rays render
        what they are given, and get_rays_directions stays world-space."""
        if space not in _RAY_SPACES:
            raise ValueError(f"unknown ray space {space!r}: expected one of {sorted(_RAY_SPACES)}")
        _lib.check(self.lib.nerf_ctx_set_ray_space(self.h, _RAY_SPACES[space], float(ndc_near_plane)))
        self.ray_space = space
        if space == "ndc":
            self.ndc_near_plane = float(ndc_near_plane)

    def rays_to_ndc(self, rays_orig, rays_dirs, fov, ndc_near_plane: float = 1.0):
        """World rays (..., 4) of cameras looking down -z -> (rays_orig, rays_dirs) in NDC, same shape and kind (numpy or
        torch-device arrays, as get_rays_directions); ``fov`` is the field of view the rays were generated with
        (include/nerf_mi355.h: nerf_rays_to_ndc has the formulas)."""
        arr = self._arrays(rays_orig, rays_dirs)
        shape = tuple(rays_orig.shape)
        if shape != tuple(rays_dirs.shape) or not shape or shape[-1] != 4:
            raise ValueError(f"rays must be two (..., 4) arrays of one shape, got {shape} and {tuple(rays_dirs.shape)}")
        n = int(np.prod(shape[:-1], dtype=np.int64))
        po, pd = arr.inp(_reshape(rays_orig, (n, 4)), (n, 4)), arr.inp(_reshape(rays_dirs, (n, 4)), (n, 4))
        oo, poo = arr.out(shape)
        od, pod = arr.out(shape)
        _lib.check(self.lib.nerf_rays_to_ndc(self.h, po, pd, n, float(fov), float(ndc_near_plane), poo, pod, arr.mem))
        return oo, od

    def set_scene_box(self, lo, hi=None) -> None:
        """An axis-aligned box ``lo[3] < hi[3]`` in the space of the rays the depth kernel sees (world rays, or NDC rays on an
        "ndc" context): every call that draws coarse depths AND has rays -- get_z_values_for_rays, render, render_image and
        its sharded form, the trainer -- then samples a ray on the part of [near, far] that lies inside the box; a ray that
        misses the box, or whose whole [near, far] lies inside, keeps the depths of a context without a box (include/nerf_mi355.h:
        nerf_ctx_set_scene_box has the rule).  ``set_scene_box(None)`` turns it off.  get_z_values has no rays and ignores it."""
        if lo is None and hi is None:
            _lib.check(self.lib.nerf_ctx_set_scene_box(self.h, None, None))
            self.scene_box, self.grid_resolution = None, 0      # the grid lives on the box
            return
        if lo is None or hi is None:
            raise ValueError("scene box: give both corners, or None to turn it off")
        lo_a, hi_a = np.asarray(lo, np.float32).ravel(), np.asarray(hi, np.float32).ravel()
        if lo_a.shape != (3,) or hi_a.shape != (3,):
            raise ValueError(f"scene box corners must have 3 components each, got {lo_a.shape[0]} and {hi_a.shape[0]}")
        # the library's own rule, checked here first so that a configuration error does not need a device call to show
        if not (np.isfinite(lo_a).all() and np.isfinite(hi_a).all() and (lo_a < hi_a).all()):
            raise RuntimeError(f"scene box needs finite lo < hi on every axis (lo {lo_a.tolist()}, hi {hi_a.tolist()})")
        _lib.check(self.lib.nerf_ctx_set_scene_box(self.h, lo_a.ctypes.data, hi_a.ctypes.data))
        self.scene_box = (tuple(float(v) for v in lo_a), tuple(float(v) for v in hi_a))
        self.grid_resolution = 0     # a new box drops the grid

    # ---- occupancy grid: R x R x R bits over the scene box (include/nerf_mi355.h: nerf_ctx_set_occupancy_grid has the rule) ----
    def set_occupancy_grid(self, grid) -> None:
        """``grid``: an (R, R, R) bool array indexed [ix, iy, iz], or the R^3 / 32 packed uint32 words (1-D), or None to clear
        it.  With a grid every call that follows the scene box samples a ray from the first occupied cell it enters to the
        last one it leaves; a ray that meets none keeps what the box alone gives it.  Needs a scene box; a new box drops it.
        The grid is a snapshot: nothing here or in the library ever rebuilds it, so after the weights change (training) it is
        stale until the caller sets or bakes it again -- training with a stale grid is the caller's choice."""
        if grid is None:
            _lib.check(self.lib.nerf_ctx_set_occupancy_grid(self.h, None, 0))
            self.grid_resolution = 0
            return
        if self.scene_box is None:
            raise RuntimeError(f"{GRID_NEEDS_BOX} (set_scene_box)")
        g = np.asarray(grid)
        if g.ndim == 3:
            words, r = pack_occupancy_grid(g), g.shape[0]
        elif g.ndim == 1 and g.dtype.kind in "ui":
            words = np.ascontiguousarray(g, dtype=np.uint32)
            r = check_grid_resolution(int(round((32 * words.size) ** (1.0 / 3.0))))
            if r ** 3 != 32 * words.size:
                raise ValueError(f"{words.size} words are no R^3 / 32 for a multiple of 4 in [4, 256]")
        else:
            raise ValueError(f"an occupancy grid is an (R, R, R) bool array or a 1-D array of packed uint32 words, got "
                             f"{g.dtype} of shape {g.shape}")
        _lib.check(self.lib.nerf_ctx_set_occupancy_grid(self.h, words.ctypes.data, r))
        self.grid_resolution = r

    def occupancy_grid(self):
        """The context's grid as an (R, R, R) bool array indexed [ix, iy, iz], or None."""
        r = C.c_int32(0)
        _lib.check(self.lib.nerf_ctx_get_occupancy_grid(self.h, None, C.addressof(r)))
        if r.value == 0:
            return None
        words = np.empty(r.value ** 3 // 32, np.uint32)
        _lib.check(self.lib.nerf_ctx_get_occupancy_grid(self.h, words.ctypes.data, C.addressof(r)))
        return unpack_occupancy_grid(words, r.value)

    def bake_occupancy_grid(self, which, resolution, sigma_threshold, samples_per_cell=1, dilate=1, seed=0) -> int:
        """Bake the grid from network ``which`` (0 coarse, 1 fine) as it is NOW, in the context's precision: a cell is occupied
        if the network's sigma exceeds ``sigma_threshold`` at its centre or at one of its ``samples_per_cell - 1`` jittered
        points; the set is grown by ``dilate`` cells (0..2).  Returns the occupied count.  See set_occupancy_grid: the grid
        is never rebuilt implicitly."""
        if self.scene_box is None:
            raise RuntimeError(f"{GRID_NEEDS_BOX} (set_scene_box)")
        r = check_grid_resolution(resolution)
        thr = float(sigma_threshold)
        if not (np.isfinite(thr) and thr > 0):
            raise ValueError(f"occupancy grid: sigma_threshold must be finite and > 0 (got {sigma_threshold!r})")
        if not 1 <= int(samples_per_cell) <= 8:
            raise ValueError(f"occupancy grid: samples_per_cell must be in 1..8 (got {samples_per_cell!r})")
        if int(dilate) not in (0, 1, 2):
            raise ValueError(f"occupancy grid: dilate must be 0, 1 or 2 (got {dilate!r})")
        count = C.c_int64(0)
        self.grid_resolution = 0
        _lib.check(self.lib.nerf_occupancy_bake(self.h, int(which), r, thr, int(samples_per_cell), int(dilate), int(seed),
                                                C.addressof(count)))
        self.grid_resolution = r
        return int(count.value)

    # ---- mesh extraction: density lattice -> isosurface -> vertex colours (include/nerf_mi355.h: nerf_isosurface has the rule) ----
    def density_lattice(self, which, n, view_dir=None, device_out=False):
        """Raw sigma of network ``which`` (0 coarse, 1 fine) at the n^3 lattice points of the scene box, n in 2..512, in the
        context's precision: an (n, n, n) float32 array indexed [iz, iy, ix] (x fastest), the sigma column of model_predict at
        the points lo + step * i, step = (hi - lo) / (n - 1).  ``view_dir``: three numbers, the view direction of every point
        (default (0, 0, 1), the bake's; ignored for n_angles == 0).  The result is a numpy array, or a torch-device tensor if
        ``view_dir`` is one or ``device_out`` is set."""
        return self._lattice("density lattice", self.lib.nerf_density_lattice, which, n, (), [(view_dir, (3,), "view_dir")],
                             view_dir, device_out)

    def _lattice(self, what, entry, which, n, channels, small, probe, device_out):
        """density_lattice and radiance_lattice: the checks, the (n, n, n) + ``channels`` output -- on the device if ``probe``
        is a torch-device tensor or ``device_out`` is set -- and the call of ``entry`` with the ``small`` host arguments
        ((value or None, shape, name), in the entry's order) between n and the output."""
        if self.scene_box is None:
            raise RuntimeError(f"a {what} needs a scene box (set_scene_box)")
        n = int(n)
        if not 2 <= n <= 512:
            raise ValueError(f"{what}: n must be in 2..512 (got {n})")
        if device_out and not (_is_torch(probe) and probe.is_cuda):
            import torch
            arr = self._arrays(torch.empty(1, device=torch.device("cuda", self.cfg.device)))   # torch's current stream
        else:
            arr = self._arrays(probe)
        host = [None if x is None else _host_floats(x, shape, name) for x, shape, name in small]
        ptrs = [None if a is None else a.ctypes.data for a in host]

        def run():
            out, p = arr.out((n, n, n) + channels)
            _lib.check(entry(self.h, int(which), n, *ptrs, p, arr.mem))
            return out
        return self._auto_call(run, arr.mem)

    def isosurface(self, sigma, lo, hi, iso, normals=True):
        """The surface sigma = iso of an (n, n, n) volume indexed [iz, iy, ix] over the box (lo, hi), n in 2..512, by marching
        tetrahedra on the device -> (vertices (V, 3) float32, triangles (T, 3) int32, normals (V, 3) float32 or None), numpy or
        torch-device arrays as ``sigma`` is.  Inside is sigma > iso; triangles are counter-clockwise seen from the outside and
        normals point from inside to outside (-gradient).  The numbering is canonical (nerf_isosurface has the rule)."""
        arr = self._arrays(sigma)
        shape = tuple(sigma.shape)
        if len(shape) != 3 or shape[0] != shape[1] or shape[0] != shape[2]:
            raise ValueError(f"sigma must be an (n, n, n) array, got {shape}")
        n = shape[0]
        ps = arr.inp(sigma, shape)
        lo_a, hi_a = _box_corners(lo, hi)
        nv, nt = C.c_int64(0), C.c_int64(0)
        _lib.check(self.lib.nerf_isosurface(self.h, ps, n, lo_a.ctypes.data, hi_a.ctypes.data, float(iso), C.byref(nv),
                                            C.byref(nt), arr.mem))
        v, t = int(nv.value), int(nt.value)
        vertices, pvx = arr.out((v, 3))
        nrm, pn = arr.out((v, 3)) if normals else (None, None)
        triangles, pt = arr.out((t, 3), np.int32)
        _lib.check(self.lib.nerf_isosurface_fetch(self.h, pvx, pn, pt, arr.mem))
        return vertices, triangles, nrm

    def mesh_colors(self, which, vertices, normals):
        """Network ``which`` at the vertices (V, 3), each seen against its normal (view direction -normal; (0, 0, 1) for a
        zero normal): (V, 3) colours in [0, 1], the sigmoid ray_marching applies.  numpy or torch-device arrays."""
        arr = self._arrays(vertices, normals)
        v = int(vertices.shape[0])
        pvx, pn = arr.inp(vertices, (v, 3)), arr.inp(normals, (v, 3))

        def run():
            out, p = arr.out((v, 3))
            _lib.check(self.lib.nerf_mesh_colors(self.h, int(which), pvx, pn, v, p, arr.mem))
            return out
        return self._auto_call(run, arr.mem)

    # ---- radiance volume: bake the network to an RGB-sigma lattice, ray-march the lattice (include/nerf_mi355.h:
    # nerf_radiance_lattice has the format, nerf_volume_sample and nerf_volume_march the rules) ----
    def radiance_lattice(self, which, n, view_dir=None, camera=None, device_out=False):
        """Network ``which`` (0 coarse, 1 fine) at the n^3 lattice points of the scene box, n in 2..512, in the context's
        precision: an (n, n, n, 4) float32 array indexed [iz, iy, ix, channel], channels 0..2 the colour after the sigmoid,
        channel 3 the density after the ReLU.  At most one of ``view_dir`` (three numbers: the view direction of every vertex)
        and ``camera`` (a (4, 4) camera-to-world matrix: every vertex gets the direction of that camera's ray through it, a
        vertex behind the camera the central ray's; refused on an "ndc" context) may be given; neither means (0, 0, 1), the
        density lattice's.  Directions are ignored for n_angles == 0.  The result is a snapshot of this network under these
        directions: a numpy array, or a torch-device tensor if ``device_out`` is set (256 MiB at n = 256, 2 GiB at n = 512:
        keep it on the device)."""
        if view_dir is not None and camera is not None:
            raise ValueError("radiance lattice: give view_dir or camera, not both")
        return self._lattice("radiance lattice", self.lib.nerf_radiance_lattice, which, n, (4,),
                             [(view_dir, (3,), "view_dir"), (camera, (4, 4), "camera")], None, device_out)

    # The volume calls below exist in two forms, for the plain (n, n, n, 4) volume and for the SH volume (n, n, n, C) further
    # down: one body each, told which by ``sh``; the library's SH entry points take the degree after n.
    @staticmethod
    def _volume_args(volume, lo, hi, what, sh):
        """(n, degree -- None for the plain format --, lo, hi as float32 (3,) arrays) of an (n, n, n, 4) volume or an SH volume
        (n, n, n, C(degree)) over (lo, hi), checked as the library checks them."""
        shape = tuple(volume.shape)
        cube = len(shape) == 4 and shape[0] == shape[1] and shape[0] == shape[2]
        if sh and not cube:
            raise ValueError(f"SH volume must be an (n, n, n, C) array, got {shape}")
        if not sh and not (cube and shape[3] == 4):
            raise ValueError(f"volume must be an (n, n, n, 4) array, got {shape}")
        degree = sh_degree_of(shape[3]) if sh else None
        if not 2 <= shape[0] <= 512:
            raise ValueError(f"{what}: n must be in 2..512 (got {shape[0]})")
        lo_a, hi_a = _box_corners(lo, hi)
        if not (np.isfinite(lo_a).all() and np.isfinite(hi_a).all() and (lo_a < hi_a).all()):
            raise ValueError(f"{what} needs finite lo < hi on every axis (lo {lo_a.tolist()}, hi {hi_a.tolist()})")
        return shape[0], degree, lo_a, hi_a

    def _volume_call(self, name, pvol, n, degree, lo_a, hi_a, *rest):
        """nerf_volume_<name>, or with a degree nerf_sh_volume_<name>, on the arguments every volume call begins with."""
        if degree is None:
            fn, head = getattr(self.lib, f"nerf_volume_{name}"), (self.h, pvol, n)
        else:
            fn, head = getattr(self.lib, f"nerf_sh_volume_{name}"), (self.h, pvol, n, degree)
        _lib.check(fn(*head, lo_a.ctypes.data, hi_a.ctypes.data, *rest))

    def _sample_volume(self, sh, volume, lo, hi, points, dirs=None):
        arr = self._arrays(volume, points, dirs)
        n, degree, lo_a, hi_a = self._volume_args(volume, lo, hi, "SH volume sample" if sh else "volume sample", sh)
        m = int(points.shape[0])
        pvol = arr.inp(volume, tuple(volume.shape))
        pp = arr.inp(points, (m, 3))
        pd = (arr.inp(dirs, (m, 3)),) if sh else ()
        out, po = arr.out((m, 4))
        self._volume_call("sample", pvol, n, degree, lo_a, hi_a, pp, *pd, m, po, arr.mem)
        return out

    def _march_volume(self, sh, volume, lo, hi, rays_orig, rays_dirs, n_steps, t_min):
        arr = self._arrays(volume, rays_orig, rays_dirs)
        n, degree, lo_a, hi_a = self._volume_args(volume, lo, hi, "SH volume march" if sh else "volume march", sh)
        steps, t = self._march_args(n_steps, t_min)
        nr = int(rays_orig.shape[0])
        pvol = arr.inp(volume, tuple(volume.shape))
        po, pd = arr.inp(rays_orig, (nr, 4)), arr.inp(rays_dirs, (nr, 4))
        rgb, p0 = arr.out((nr, 3))
        depth, p1 = arr.out((nr,))
        opacity, p2 = arr.out((nr,))
        self._volume_call("march", pvol, n, degree, lo_a, hi_a, po, pd, nr, steps, t, p0, p1, p2, arr.mem)
        return rgb, depth, opacity

    def _render_volume_image(self, sh, volume, lo, hi, c2w, fov, h, w, n_steps, t_min, ray_begin, ray_count):
        arr = self._arrays(volume)
        n, degree, lo_a, hi_a = self._volume_args(volume, lo, hi, "SH volume render" if sh else "volume render", sh)
        steps, t = self._march_args(n_steps, t_min)
        c2w_h = _host_floats(c2w, (4, 4), "c2w", exact=True)
        pvol = arr.inp(volume, tuple(volume.shape))
        lead = (int(h), int(w)) if ray_count <= 0 else (int(ray_count),)
        rgb, p0 = arr.out(lead + (3,))
        depth, p1 = arr.out(lead)
        opacity, p2 = arr.out(lead)
        self._volume_call("render_image", pvol, n, degree, lo_a, hi_a, c2w_h.ctypes.data, float(fov), int(h), int(w),
                          int(ray_begin), int(ray_count), steps, t, p0, p1, p2, arr.mem)
        return rgb, depth, opacity

    @staticmethod
    def _march_args(n_steps, t_min):
        if int(n_steps) != n_steps or n_steps < 1:
            raise ValueError(f"volume march: n_steps must be an integer >= 1 (got {n_steps!r})")
        t = float(t_min)
        if not 0.0 <= t < 1.0:                  # a NaN fails both comparisons
            raise ValueError(f"volume march: t_min must be in [0, 1) (got {t_min!r})")
        return int(n_steps), t

    def sample_volume(self, volume, lo, hi, points):
        """The (n, n, n, 4) ``volume`` over the box (lo, hi) at ``points`` (M, 3), trilinear -> (M, 4); numpy or torch-device
        arrays.  A point outside the box takes the value of the nearest face, a NaN coordinate gives NaN
        (nerf_volume_sample has the rule).  A numpy volume is staged to the device on every call: keep it on the device."""
        return self._sample_volume(False, volume, lo, hi, points)

    def march_volume(self, volume, lo, hi, rays_orig, rays_dirs, n_steps, t_min=0.0):
        """Rays (N, 4) marched through the (n, n, n, 4) ``volume`` over the box (lo, hi) in ``n_steps`` equal steps of the
        part of [near, far] each ray spends inside the box -> (rgb (N, 3), depth (N,), opacity (N,)).  rgb is premultiplied: a
        ray may leave the box partly transparent, and blending over a background by ``opacity`` is the caller's business.  A
        ray that misses the box gives zeros.  ``t_min`` in [0, 1): a ray stops once its transmittance falls below it, which
        changes rgb and opacity by at most t_min (nerf_volume_march has the rule).  A numpy volume is staged to the device on
        every call: keep it on the device."""
        return self._march_volume(False, volume, lo, hi, rays_orig, rays_dirs, n_steps, t_min)

    def render_volume_image(self, volume, lo, hi, c2w, fov, h, w, n_steps, t_min=0.0, ray_begin=0, ray_count=0):
        """march_volume of the rays render_image makes for camera ``c2w`` (through rays_to_ndc on an "ndc" context), generated
        on the device -> (rgb, depth, opacity) shaped (h, w, ...), or (ray_count, ...) for a slab of rays; equal to
        get_rays_directions + march_volume bit for bit.  A numpy volume is staged to the device on every call: keep it on the
        device."""
        return self._render_volume_image(False, volume, lo, hi, c2w, fov, h, w, n_steps, t_min, ray_begin, ray_count)

    # ---- SH radiance volume: view-dependent colour as spherical harmonics per vertex (include/nerf_mi355.h:
    # nerf_sh_radiance_lattice has the format, nerf_sh_volume_sample the rule) ----
    def sh_radiance_lattice(self, which, n, degree, dirs=None, proj=None, device_out=False):
        """Network ``which`` baked onto the n^3 lattice of the scene box as spherical harmonics of degree ``degree`` (0..3) in the
        view direction: an (n, n, n, C) float32 array indexed [iz, iy, ix, channel], C = 4 / 16 / 28 / 52, channel 3 k + c the
        coefficient of basis function k for colour c, channel 3 K the density after the ReLU, zeros after it.  ``dirs`` (D, 3)
        and ``proj`` (K, D), D in 1..64, are the projection table: the network is evaluated at every vertex along each of
        ``dirs`` as given, and the coefficients are ``proj`` times the D colours.  Default: ``sh_quadrature(degree)``, a
        full-sphere quadrature; ``sh_least_squares(degree, dirs)`` fits a caller's own directions.  One bake answers for every
        pose -- for the unit direction d / |d|, while the network sees the ray generator's un-normalised directions, and a
        full-sphere table includes directions no camera saw.  n^3 C 4 bytes (1.75 GiB at n = 256, degree 2): a numpy array, or
        a torch-device tensor if ``device_out`` is set."""
        degree = check_sh_degree(degree)
        if (dirs is None) != (proj is None):
            raise ValueError("SH radiance lattice: give both dirs and proj, or neither")
        if dirs is None:
            dirs, proj = sh_quadrature(degree)
        k = sh_basis_count(degree)
        dirs_a = np.ascontiguousarray(dirs.detach().cpu().numpy() if _is_torch(dirs) else dirs, dtype=np.float32)
        if dirs_a.ndim != 2 or dirs_a.shape[1] != 3 or not 1 <= dirs_a.shape[0] <= SH_MAX_DIRS:
            raise ValueError(f"SH radiance lattice: dirs must be (D, 3) with D in 1..{SH_MAX_DIRS}, got {dirs_a.shape}")
        d = dirs_a.shape[0]
        proj_a = _host_floats(proj, (k, d), "proj", exact=True)
        if not (np.isfinite(dirs_a).all() and np.isfinite(proj_a).all()):
            raise ValueError("SH radiance lattice: dirs and proj must be finite")
        if not dirs_a.any(axis=1).all():
            raise ValueError(f"SH radiance lattice: dirs[{int(np.argmin(dirs_a.any(axis=1)))}] is the zero vector")

        def entry(h, which_, n_, out, mem):
            return self.lib.nerf_sh_radiance_lattice(h, which_, n_, degree, dirs_a.ctypes.data, proj_a.ctypes.data, d, out, mem)
        return self._lattice("SH radiance lattice", entry, which, n, (sh_texel_floats(degree),), [], None, device_out)

    def sample_sh_volume(self, volume, lo, hi, points, dirs):
        """The SH ``volume`` (n, n, n, C) over the box (lo, hi) at ``points`` (M, 3) seen along ``dirs`` (M, 3, any length; a zero
        or non-finite direction counts as (0, 0, 1)) -> (M, 4): the colour, clamped to [0, 1], and the density; numpy or
        torch-device arrays (nerf_sh_volume_sample has the rule).  The degree follows from C."""
        return self._sample_volume(True, volume, lo, hi, points, dirs)

    def march_sh_volume(self, volume, lo, hi, rays_orig, rays_dirs, n_steps, t_min=0.0):
        """march_volume through an SH ``volume`` (n, n, n, C): every sample's colour is the volume's towards the ray's own
        direction -> (rgb (N, 3), depth (N,), opacity (N,)) (nerf_sh_volume_march)."""
        return self._march_volume(True, volume, lo, hi, rays_orig, rays_dirs, n_steps, t_min)

    def render_sh_volume_image(self, volume, lo, hi, c2w, fov, h, w, n_steps, t_min=0.0, ray_begin=0, ray_count=0):
        """render_volume_image through an SH ``volume`` (n, n, n, C): equal to get_rays_directions + march_sh_volume bit for
        bit (nerf_sh_volume_render_image)."""
        return self._render_volume_image(True, volume, lo, hi, c2w, fov, h, w, n_steps, t_min, ray_begin, ray_count)

    def ray_occupancy_bounds(self, rays_orig, rays_dirs):
        """Rays (N,4) -> (bounds (N,2) float32, state (N,) int32) under the context's box, grid and bounds: state 2 and the
        grid's interval, state 1 and the box's for a ray only the box narrows, state 0 and (near, far) for any other
        (nerf_ray_occupancy_bounds: the device function behind the depth kernels)."""
        arr = self._arrays(rays_orig, rays_dirs)
        n = int(rays_orig.shape[0])
        po, pd = arr.inp(rays_orig, (n, 4)), arr.inp(rays_dirs, (n, 4))
        bounds, pb = arr.out((n, 2))
        state, ps = arr.out((n,), np.int32)
        _lib.check(self.lib.nerf_ray_occupancy_bounds(self.h, po, pd, n, pb, ps, arr.mem))
        return bounds, state

    # ---- sample culling under the grid (include/nerf_mi355.h: nerf_ctx_set_sample_culling has the rule) ----
    def set_sample_culling(self, on) -> None:
        """With a grid, the samples of a render pass that lie in empty cells skip the network and count as raw output
        (0, 0, 0, 0); samples outside the box are kept.  Off by default; it may be set with or without a grid and acts only
        while the context holds one.  render_rays, render, render_image and the sharded calls follow it; the trainer (and so
        DietNeRF's consistency render) ignores it.  A culled call reads a row count per network pass: it synchronises."""
        _lib.check(self.lib.nerf_ctx_set_sample_culling(self.h, int(bool(on))))
        self.sample_culling = bool(on)

    def set_train_sample_culling(self, on) -> None:
        """The trainer's own switch (nerf_ctx_set_train_sample_culling has the rule): with a grid, the samples of a training
        pass that lie in empty cells are never network rows, forward or backward, and count as the constant raw output
        (0, 0, 0, 0); culled cells receive no gradient.  Off by default, independent of set_sample_culling; it may be set with
        or without a grid or a running trainer and acts only while the context holds a grid.  train_step, train_gradients,
        train_render_gradients and train_render_forward / _backward follow it.  A culled training call reads a row count per
        network pass: it synchronises."""
        _lib.check(self.lib.nerf_ctx_set_train_sample_culling(self.h, int(bool(on))))
        self._train_sample_culling = bool(on)

    @property
    def train_sample_culling(self) -> bool:
        """Whether set_train_sample_culling is on."""
        return self._train_sample_culling

    def sample_occupancy(self, rays_orig, rays_dirs, z_values):
        """Rays (N,4), depths (N,S) -> the culling verdict (N,S) int32, 1 kept / 0 culled, under the context's box and grid
        (nerf_sample_occupancy: the device function behind the render path)."""
        arr = self._arrays(rays_orig, rays_dirs, z_values)
        n, s = int(z_values.shape[0]), int(z_values.shape[1])
        po, pd, pz = arr.inp(rays_orig, (n, 4)), arr.inp(rays_dirs, (n, 4)), arr.inp(z_values, (n, s))
        keep, pk = arr.out((n, s), np.int32)
        _lib.check(self.lib.nerf_sample_occupancy(self.h, po, pd, pz, n, s, pk, arr.mem))
        return keep

    def read_culling(self) -> Tuple[int, int]:
        """(samples, kept) summed over all culled network passes since the last call; clears both."""
        samples, kept = C.c_int64(), C.c_int64()
        _lib.check(self.lib.nerf_ctx_read_culling(self.h, C.byref(samples), C.byref(kept)))
        return samples.value, kept.value

    def read_culling_timing(self) -> Tuple[Tuple[float, float, float, float], int]:
        """With enable_timing: ((verdict + scan, host read of the row count, gather, expand) in ms, culled passes) since the
        last call (synchronises); the network itself is read_timing's.  Call it BEFORE read_timing, which clears these too."""
        ms, n = (C.c_double * 4)(), C.c_int64()
        _lib.check(self.lib.nerf_ctx_read_culling_timing(self.h, ms, C.byref(n)))
        return tuple(ms), n.value

    def ray_box_bounds(self, rays_orig, rays_dirs):
        """Rays (N,4) -> (bounds (N,2) float32, narrowed (N,) int32) under the context's box and bounds: (a, b) of a ray the
        box narrows, (near, far) of any other (nerf_ray_box_bounds: the device function the depth kernels call)."""
        arr = self._arrays(rays_orig, rays_dirs)
        n = int(rays_orig.shape[0])
        po, pd = arr.inp(rays_orig, (n, 4)), arr.inp(rays_dirs, (n, 4))
        bounds, pb = arr.out((n, 2))
        narrowed, pn = arr.out((n,), np.int32)
        _lib.check(self.lib.nerf_ray_box_bounds(self.h, po, pd, n, pb, pn, arr.mem))
        return bounds, narrowed

    def get_z_values_for_rays(self, rays_orig, rays_dirs, n_samples, uniform_values=None, seed=0, ray_base=0):
        """The coarse depths (N, n_samples) render and the trainer draw for these rays (N,4) at the context's bounds: get_z_values
        for callers that have rays -- it follows the sampling mode and the scene box."""
        arr = self._arrays(rays_orig, rays_dirs, uniform_values)
        n = int(rays_orig.shape[0])
        po, pd = arr.inp(rays_orig, (n, 4)), arr.inp(rays_dirs, (n, 4))
        pu = arr.inp(uniform_values, (n, n_samples))
        out, p = arr.out((n, n_samples))
        _lib.check(self.lib.nerf_get_z_values_rays(self.h, po, pd, n, n_samples, pu, seed, ray_base, p, arr.mem))
        return out

    def set_precision(self, precision: str) -> None:
        """"auto", "fp32" (exact fp32 MFMA), "f16x3" (3-pass split-fp16 MFMA, fp32 accumulate), "bf16x3" (3-pass split-bf16
        MFMA, fp32 accumulate: fp32's range) or "f16".  Works at any time: every mode's operand streams stay resident."""
        _lib.check(self.lib.nerf_ctx_set_precision(self.h, _PRECISIONS[precision]))
        self.cfg.precision = _PRECISIONS[precision]
        self.precision, self._auto_fp32, self._auto_unchecked = precision, False, False

    # ---- precision="auto": f16x3 by default, exact fp32 (n_pos_enc_xyz 6..10: bf16x3) for a weight set that needs it ----
    def _auto_new_weights(self) -> None:
        """The fallback is per weight set (src/NeRF.py:190-246 renders whatever the model holds): new weights try f16x3 again."""
        if self.precision == "auto" and self._auto_fp32:
            _lib.check(self.lib.nerf_ctx_set_precision(self.h, NERF_PRECISION_F16X3))
            self.cfg.precision, self._auto_fp32 = NERF_PRECISION_F16X3, False

    def _auto_to_fp32(self) -> None:
        # the wide-PE networks (n_pos_enc_xyz 6..10) have no exact-fp32 kernel: their fallback is the bf16x3 mode
        to = NERF_PRECISION_FP32 if self.cfg.n_pos_enc_xyz <= 5 else _lib.NERF_PRECISION_BF16X3
        _lib.check(self.lib.nerf_ctx_set_precision(self.h, to))
        self.cfg.precision, self._auto_fp32, self._auto_unchecked = to, True, False

    def _auto_call(self, call, mem):
        """Run ``call`` (one path function that evaluates a network).  Under precision="auto" a host-memory call -- which
        is synchronous on return anyway -- then reads the library's non-finite counter (a device counter the fused kernels
        add to: one 8-byte copy, no extra synchronisation); a non-zero count means activations left the fp16 range in the
        f16x3 kernels, so the call is repeated in exact fp32 (bf16x3 for n_pos_enc_xyz 6..10; same draws: same seed) and the
        context stays there until its weights change.  Device-resident calls are asynchronous and are NOT checked one by one (that would drain the
        queue per call): ``auto_check()`` looks at the counter when the caller synchronises (video.render_video does)."""
        out = call()
        if self.precision != "auto" or self._auto_fp32:
            return out
        if mem != NERF_MEM_HOST:
            self._auto_unchecked = True
            return out
        if self.read_nonfinite() > 0:
            self._auto_to_fp32()
            self.auto_fallbacks += 1
            out = call()
        self._auto_unchecked = False
        return out

    def auto_check(self) -> bool:
        """precision="auto" after device-resident (asynchronous) calls: synchronise, read the non-finite counter and, if it
        is non-zero, switch to exact fp32 for this weight set.  True = the caller should render those calls again."""
        if self.precision != "auto" or self._auto_fp32 or not self._auto_unchecked:
            return False
        self._auto_unchecked = False
        if self.read_nonfinite() > 0:
            self._auto_to_fp32()
            self.auto_fallbacks += 1
            return True
        return False

    def synchronize(self) -> None:
        _lib.check(self.lib.nerf_ctx_synchronize(self.h))

    def use_torch_stream(self) -> None:
        """Enqueue on torch's current stream, so torch events/ops order with the kernels."""
        import torch
        cur = torch.cuda.current_stream().cuda_stream
        _lib.check(self.lib.nerf_ctx_set_stream(self.h, C.c_void_p(cur)))
        self._stream = cur

    def read_nonfinite(self) -> int:
        """Rows with a non-finite network output since the last call (synchronises).  Non-zero in the
        f16x3 mode means activations left the fp16 range: use precision="bf16x3" or "fp32" for this model."""
        n = C.c_int64()
        _lib.check(self.lib.nerf_ctx_read_nonfinite(self.h, C.byref(n)))
        return n.value

    # ---- multi-GPU assembly through the C ABI (RCCL all-gather inside the library) ----
    @staticmethod
    def comm_unique_id() -> bytes:
        """An RCCL unique id (rank 0 creates it and hands it to the other ranks)."""
        buf = C.create_string_buffer(128)
        _lib.check(_lib.load().nerf_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, unique_id: bytes, rank: int, world: int) -> None:
        buf = C.create_string_buffer(bytes(unique_id), 128)
        self.comm_world = 0
        _lib.check(self.lib.nerf_comm_init(self.h, buf, rank, world))
        self.comm_world = world

    def comm_init_from_torch(self, group=None) -> None:
        """Join the ranks of an initialised torch.distributed group: rank 0 draws the id, the group (any backend --
        it only carries 128 bytes) hands it to the others.  One process per GPU: RCCL refuses two ranks on a device."""
        import torch.distributed as dist
        rank, world = dist.get_rank(group), dist.get_world_size(group)
        box = [self.comm_unique_id() if rank == 0 else None]
        dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
        self.comm_init(box[0], rank, world)

    def comm_destroy(self) -> None:
        self.comm_world = 0
        _lib.check(self.lib.nerf_comm_destroy(self.h))

    def render_image_sharded(self, c2w, fov, h, w, batch, n_c, n_f, seed=0, device_out=False, outputs=None,
                             want_depth=False):
        """This rank renders its slab; ONE ncclAllGather per requested output inside the library assembles the whole image
        on every rank.  ``outputs=None``: rgb alone -> (h,w,3) (nerf_render_image_sharded).  ``outputs="all"``: the
        6-tuple of NeRF.render_image (+ depth with ``want_depth``); ``outputs="rgb_depth"``: (rgb, depth), what the video
        loop needs per frame (src/ExecutionRun.py:339-356) -- through nerf_render_image_sharded_outputs (ABI 4)."""
        c2w_h = np.ascontiguousarray(np.asarray(c2w, np.float32))
        if device_out:
            import torch
            arr = self._arrays(torch.empty(1, device=torch.device("cuda", self.cfg.device)))   # torch's current stream
        else:
            arr = self._arrays()
        if outputs is None:
            out, ptr = arr.out((h, w, 3))
            _lib.check(self.lib.nerf_render_image_sharded(self.h, c2w_h.ctypes.data, float(fov), h, w, batch or 0, n_c, n_f,
                                                          seed, ptr, arr.mem))
            return out
        fine = n_f > 0 and self.loaded[NERF_NET_FINE]
        s = n_c + n_f if fine else n_c
        if outputs == "rgb_depth":
            rgb, p0 = arr.out((h, w, 3))
            d, p6 = arr.out((h, w))
            o, res = NerfOutputs(p0, None, None, None, None, None, p6), (rgb, d)
        elif outputs == "all":
            o, res = self._outputs(arr, h * w, s, want_depth, (h, w))
            res = res if want_depth else res[:6]
        else:
            raise ValueError('outputs must be None, "all" or "rgb_depth"')
        _lib.check(self.lib.nerf_render_image_sharded_outputs(self.h, c2w_h.ctypes.data, float(fov), h, w, batch or 0, n_c,
                                                              n_f if fine else 0, seed, C.byref(o), arr.mem))
        return res

    # ---- training (NeRF.train_step, src/NeRF.py:136-178) ----
    def train_begin(self, learning_rate: float, beta_1: float = 0.9, beta_2: float = 0.999, epsilon: float = 1e-7,
                    sampler_gradient: bool = True, mixed_float16: bool = False, initial_loss_scale: float = 0.0,
                    dynamic_growth_steps: int = 0) -> None:
        """Adam(lr) as model.compile(optimizer=Adam(optimizer_lr)) (src/ExecutionRun.py:226-227).
        ``mixed_float16=True`` is the reference's production policy (src/ExecutionRun.py:220-221): fp16 compute with
        fp32 master weights and Keras' dynamic loss scaling (LossScaleOptimizer; src/NeRF.py:159-163)."""
        cfg = NerfTrainConfig(learning_rate, beta_1, beta_2, epsilon, 1 if sampler_gradient else 0,
                              1 if mixed_float16 else 0, float(initial_loss_scale), int(dynamic_growth_steps))
        _lib.check(self.lib.nerf_train_begin(self.h, C.byref(cfg)))
        self._train_ray_gradients = False      # (nerf_train_begin leaves the switch off)

    def train_loss_scale(self) -> Tuple[float, int, int]:
        """(current loss scale, optimizer steps applied, steps skipped) -- (1, n, 0) under the fp32 policy."""
        s, a, k = C.c_float(), C.c_int64(), C.c_int64()
        _lib.check(self.lib.nerf_train_loss_scale(self.h, C.byref(s), C.byref(a), C.byref(k)))
        return float(s.value), int(a.value), int(k.value)

    def train_read_metric_sums(self) -> Tuple[Dict[str, float], int]:
        """Sums of the step metrics since the last read and the number of steps they cover (kept on the device; this
        synchronises and clears them): what a training loop needs for Keras' per-epoch means without reading metrics
        every step (nerf_train_read_metric_sums, ABI 4)."""
        sums, steps = (C.c_double * 3)(), C.c_int64()
        _lib.check(self.lib.nerf_train_read_metric_sums(self.h, sums, C.byref(steps)))
        out = {"loss": float(sums[0]), "psnr_coarse": float(sums[1])}
        if self.loaded[1]:
            out["psnr_fine"] = float(sums[2])
        return out, int(steps.value)

    def train_end(self) -> None:
        _lib.check(self.lib.nerf_train_end(self.h))

    def train_set_learning_rate(self, learning_rate: float) -> None:
        _lib.check(self.lib.nerf_train_set_learning_rate(self.h, learning_rate))

    def train_set_loss_weights(self, coarse_mse_weight: float = 1.0, fine_mse_weight: float = 1.0) -> None:
        """Ray loss = coarse_mse_weight * MSE(coarse) + fine_mse_weight * MSE(fine).  (1, 1) = NeRF.train_step
        (src/NeRF.py:151,157; what train_begin leaves); DietNeRF's tape differentiates (2, 1) (src/DietNeRF.py:160-170)."""
        _lib.check(self.lib.nerf_train_set_loss_weights(self.h, float(coarse_mse_weight), float(fine_mse_weight)))

    def train_set_distortion_weights(self, coarse: float = 0.0, fine: float = 0.0) -> None:
        """Objective += coarse * L(coarse pass) + fine * L(fine pass), L the batch mean of the distortion loss of mip-NeRF 360
        on the pass's compositing weights (nerf_train_set_distortion_weights).  (0, 0) = off, what train_begin leaves.  Acts on
        train_step / train_gradients only: the backward passes through ``render`` (train_render_*) ignore it."""
        _lib.check(self.lib.nerf_train_set_distortion_weights(self.h, float(coarse), float(fine)))

    def train_read_distortion_sums(self) -> Tuple[Dict[str, float], int]:
        """Sums of the unweighted distortion losses of the steps that ran under a non-zero weight since the last read, and
        how many such steps there were (kept on the device; this synchronises and clears them)."""
        sums, steps = (C.c_double * 2)(), C.c_int64()
        _lib.check(self.lib.nerf_train_read_distortion_sums(self.h, sums, C.byref(steps)))
        return {"distortion_coarse": float(sums[0]), "distortion_fine": float(sums[1])}, int(steps.value)

    def distortion_loss(self, weights, z_values):
        """The bare distortion-loss operator: weights, z_values (N, S), depths sorted along each ray ->
        (loss_per_ray (N,), d_weights (N, S), d_z (N, S)), per ray and unscaled; t is measured between the context's bounds."""
        arr = self._arrays(weights, z_values)
        n, s = tuple(weights.shape)
        pw, pz = arr.inp(weights, (n, s)), arr.inp(z_values, (n, s))
        loss, pl = arr.out((n,))
        dw, pdw = arr.out((n, s))
        dz, pdz = arr.out((n, s))
        _lib.check(self.lib.nerf_distortion_loss(self.h, pw, pz, n, s, pl, pdw, pdz, arr.mem))
        return loss, dw, dz

    def _train_inputs(self, rays_orig, rays_dirs, real_rgb, n_c, n_f, u_coarse, u_fine):
        arr = self._arrays(rays_orig, rays_dirs, real_rgb)
        n = int(rays_orig.shape[0])
        ptrs = (arr.inp(rays_orig, (n, 4)), arr.inp(rays_dirs, (n, 4)), arr.inp(real_rgb, (n, 3)))
        uc = arr.inp(u_coarse, (n, n_c)) if u_coarse is not None else None
        uf = arr.inp(u_fine, (n, n_f)) if (u_fine is not None and n_f > 0) else None
        return arr, n, ptrs, uc, uf

    def train_step(self, rays_orig, rays_dirs, real_rgb, n_c, n_f, u_coarse=None, u_fine=None, seed=0,
                   want_metrics=True) -> Optional[Dict[str, float]]:
        """One optimizer step on a batch of rays -> {"loss", "psnr_coarse", "psnr_fine"} (src/NeRF.py:166-177)."""
        arr, n, (po, pd, pt), uc, uf = self._train_inputs(rays_orig, rays_dirs, real_rgb, n_c, n_f, u_coarse, u_fine)
        m = (C.c_float * 3)()
        _lib.check(self.lib.nerf_train_step(self.h, po, pd, pt, n, n_c, n_f, uc, uf, seed,
                                            C.cast(m, C.c_void_p) if want_metrics else None, arr.mem))
        self._auto_new_weights()
        return _metrics(m, n_f > 0 and self.loaded[1]) if want_metrics else None

    def train_gradients(self, rays_orig, rays_dirs, real_rgb, n_c, n_f, u_coarse=None, u_fine=None, seed=0,
                        want_metrics=True, want_blobs=True):
        """Gradients without the update -> (metrics, grad_coarse blob, grad_fine blob | None).  The gradients stay in the
        context either way; ``want_blobs=False`` skips the copies, ``want_metrics=False`` the synchronisation (-> None)."""
        arr, n, (po, pd, pt), uc, uf = self._train_inputs(rays_orig, rays_dirs, real_rgb, n_c, n_f, u_coarse, u_fine)
        fine = n_f > 0 and self.loaded[1]
        gc, pgc = arr.out((self.blob_size(),)) if want_blobs else (None, None)
        gf, pgf = arr.out((self.blob_size(),)) if fine and want_blobs else (None, None)
        m = (C.c_float * 3)()
        _lib.check(self.lib.nerf_train_gradients(self.h, po, pd, pt, n, n_c, n_f, uc, uf, seed, pgc, pgf,
                                                 C.cast(m, C.c_void_p) if want_metrics else None, arr.mem))
        return (_metrics(m, fine) if want_metrics else None), gc, gf

    def train_render_gradients(self, rays_orig, rays_dirs, d_rgb, n_c, n_f, u_coarse=None, u_fine=None, seed=0,
                               ray_base=0, accumulate=False):
        """Backward through ``NeRF.render`` (src/NeRF.py:109-134; what DietNeRF's consistency loss differentiates,
        src/DietNeRF.py:204-222): ``d_rgb`` (N,3) = dL/d(render(...)[0]) -> (rgb (N,3) of the re-run forward,
        grad_coarse blob, grad_fine blob | None).  ``accumulate=True`` adds to the gradients the last
        ``train_gradients`` left in the context (then ``train_apply()`` steps on the sum)."""
        arr, n, (po, pd, pg), uc, uf = self._train_inputs(rays_orig, rays_dirs, d_rgb, n_c, n_f, u_coarse, u_fine)
        fine = n_f > 0 and self.loaded[1]
        rgb, prgb = arr.out((n, 3))
        gc, pgc = arr.out((self.blob_size(),))
        gf, pgf = arr.out((self.blob_size(),)) if fine else (None, None)
        _lib.check(self.lib.nerf_train_render_gradients(self.h, po, pd, pg, n, n_c, n_f, uc, uf, seed, ray_base,
                                                        1 if accumulate else 0, prgb, pgc, pgf, arr.mem))
        return rgb, gc, gf

    def train_render_forward(self, slot: int, rays_orig, rays_dirs, n_c, n_f, u_coarse=None, u_fine=None, seed=0, ray_base=0):
        """First half of ``train_render_gradients`` with the activations KEPT in ``slot`` (nerf_train_render_forward, ABI 5):
        -> rgb (N,3) of this batch -- the forward of the tape itself.  For callers whose d_rgb needs the whole image first
        (DietNeRF's embedding network): forward every batch into its own slot, build d_rgb, then ``train_render_backward``
        per slot; the image is not rendered a second time.  An optimizer step invalidates all slots."""
        arr = self._arrays(rays_orig, rays_dirs)
        n = int(rays_orig.shape[0])
        po, pd = arr.inp(rays_orig, (n, 4)), arr.inp(rays_dirs, (n, 4))
        uc = arr.inp(u_coarse, (n, n_c)) if u_coarse is not None else None
        uf = arr.inp(u_fine, (n, n_f)) if (u_fine is not None and n_f > 0) else None
        rgb, prgb = arr.out((n, 3))
        _lib.check(self.lib.nerf_train_render_forward(self.h, int(slot), po, pd, n, n_c, n_f, uc, uf, seed, ray_base, prgb,
                                                      arr.mem))
        self._slot_fine[int(slot)] = n_f > 0 and self.loaded[1]
        self._slot_rays[int(slot)] = n
        return rgb

    def train_render_backward(self, slot: int, d_rgb, accumulate=False, want_blobs=True):
        """Second half: ``d_rgb`` (N,3) for the batch kept in ``slot`` -> (grad_coarse blob, grad_fine blob | None) copies (or
        (None, None)); the gradients stay in / are added to the context's blobs exactly as ``train_render_gradients`` leaves
        them (bit-identical).  Consumes the slot."""
        arr = self._arrays(d_rgb)
        pg = arr.inp(d_rgb)
        fine = self._slot_fine.get(int(slot), False)
        gc, pgc = arr.out((self.blob_size(),)) if want_blobs else (None, None)
        gf, pgf = arr.out((self.blob_size(),)) if want_blobs and fine else (None, None)
        _lib.check(self.lib.nerf_train_render_backward(self.h, int(slot), pg, 1 if accumulate else 0, pgc, pgf, arr.mem))
        return gc, gf

    _TRAIN_OUTPUTS = ("rgb", "depth", "weights", "z")

    def train_render_forward_outputs(self, slot: int, rays_orig, rays_dirs, n_c, n_f, u_coarse=None, u_fine=None, seed=0,
                                     ray_base=0, outputs=_TRAIN_OUTPUTS) -> Dict[str, object]:
        """``train_render_forward`` with every output a loss can be written on (nerf_train_render_forward_outputs): -> dict of
        the ``outputs`` asked for, of the LAST pass -- ``rgb`` (N,3), the same bits as ``train_render_forward``; ``depth`` (N,)
        = sum_s w_s z_s; ``weights`` and ``z`` (N,S), S = n_c + n_f with a fine pass (z merged and sorted), else n_c.  The
        slot is the same slot: ``train_render_backward`` or ``train_render_backward_outputs`` consumes it."""
        bad = [k for k in outputs if k not in self._TRAIN_OUTPUTS]
        if bad or not len(outputs):
            raise ValueError(f"outputs must name some of {self._TRAIN_OUTPUTS}, got {tuple(outputs)}")
        arr = self._arrays(rays_orig, rays_dirs)
        n = int(rays_orig.shape[0])
        po, pd = arr.inp(rays_orig, (n, 4)), arr.inp(rays_dirs, (n, 4))
        uc = arr.inp(u_coarse, (n, n_c)) if u_coarse is not None else None
        uf = arr.inp(u_fine, (n, n_f)) if (u_fine is not None and n_f > 0) else None
        fine = n_f > 0 and self.loaded[1]
        s = n_c + n_f if fine else n_c
        shapes = {"rgb": (n, 3), "depth": (n,), "weights": (n, s), "z": (n, s)}
        got = {k: arr.out(shapes[k]) for k in self._TRAIN_OUTPUTS if k in outputs}
        o = _lib.NerfTrainOutputs(*[got[k][1] if k in got else None for k in self._TRAIN_OUTPUTS])
        _lib.check(self.lib.nerf_train_render_forward_outputs(self.h, int(slot), po, pd, n, n_c, n_f, uc, uf, seed, ray_base,
                                                              C.byref(o), arr.mem))
        self._slot_fine[int(slot)] = fine
        self._slot_rays[int(slot)] = n
        return {k: v[0] for k, v in got.items()}

    def train_set_ray_gradients(self, on) -> None:
        """Switches the ray gradients of ``train_render_backward_outputs(..., want_rays=True)`` and of ``render_with_grad`` on
        or off on a running trainer (nerf_train_set_ray_gradients has the rules): both networks' backward streams are
        re-packed with or without the encoding tiles.  Off by default, and off again after every ``train_begin``; while it
        is off nothing changes.  The fused trainer only."""
        _lib.check(self.lib.nerf_train_set_ray_gradients(self.h, int(bool(on))))
        self._train_ray_gradients = bool(on)

    @property
    def train_ray_gradients(self) -> bool:
        """Whether train_set_ray_gradients is on."""
        return self._train_ray_gradients

    def train_render_backward_outputs(self, slot: int, d_rgb=None, d_depth=None, d_weights=None, d_z=None, accumulate=False,
                                      want_blobs=True, want_rays=False):
        """``train_render_backward`` with a cotangent for every output of ``train_render_forward_outputs``
        (nerf_train_render_backward_outputs): any of ``d_rgb`` (N,3), ``d_depth`` (N,), ``d_weights``, ``d_z`` (N,S) may be
        None (= zero), not all four -> (grad_coarse blob, grad_fine blob | None) copies (or (None, None)).  With ``d_rgb``
        alone it is ``train_render_backward``, bit for bit.  ``d_z`` and the depth's own dependence on z reach the networks
        only with a fine pass under ``sampler_gradient`` (through the n_f new depths; the coarse depths are data).  Under
        mixed_float16 pass UNSCALED cotangents: the library applies the loss scale.  Consumes the slot.
        ``want_rays=True`` (nerf_train_render_backward_rays; needs ``train_set_ray_gradients(True)``) -> (grad_coarse,
        grad_fine, d_rays_orig, d_rays_dirs): the gradients of the same scalar with respect to the (N,4) rays the slot's
        forward received, component 3 zero -- through the sample points of every pass that takes part and through the
        view-direction input; the coarse depths, the bounds and what a box or grid derives from the ray are data."""
        arr = self._arrays(d_rgb, d_depth, d_weights, d_z)
        g = _lib.NerfRenderGrads(arr.inp(d_rgb), arr.inp(d_depth), arr.inp(d_weights), arr.inp(d_z))
        fine = self._slot_fine.get(int(slot), False)
        gc, pgc = arr.out((self.blob_size(),)) if want_blobs else (None, None)
        gf, pgf = arr.out((self.blob_size(),)) if want_blobs and fine else (None, None)
        if want_rays:
            n = self._slot_rays.get(int(slot))
            if n is None:
                raise RuntimeError(f"slot {int(slot)} holds no forward pass of train_render_forward_outputs")
            g_o, pgo = arr.out((n, 4))
            g_d, pgd = arr.out((n, 4))
            _lib.check(self.lib.nerf_train_render_backward_rays(self.h, int(slot), C.byref(g), 1 if accumulate else 0, pgc, pgf,
                                                                pgo, pgd, arr.mem))
            return gc, gf, g_o, g_d
        _lib.check(self.lib.nerf_train_render_backward_outputs(self.h, int(slot), C.byref(g), 1 if accumulate else 0, pgc, pgf,
                                                               arr.mem))
        return gc, gf

    def ray_position_grads(self, d_points, z_values):
        """The bare per-ray reduction of the ray gradients (nerf_ray_position_grads): d_points (N,S,3) = dL/dp per sample,
        z_values (N,S) -> (d_rays_orig, d_rays_dirs) (N,4): sum_s d_points and sum_s z d_points, component 3 zero."""
        arr = self._arrays(d_points, z_values)
        n, s = tuple(z_values.shape)
        pp, pz = arr.inp(d_points, (n, s, 3)), arr.inp(z_values, (n, s))
        g_o, pgo = arr.out((n, 4))
        g_d, pgd = arr.out((n, 4))
        _lib.check(self.lib.nerf_ray_position_grads(self.h, pp, pz, n, s, pgo, pgd, arr.mem))
        return g_o, g_d

    def render_output_grads(self, weights, z_values, d_depth=None, d_weights=None, d_z=None):
        """The bare fold of the depth / weights / z cotangents (nerf_render_output_grads): weights, z_values (N,S) and any of
        d_depth (N,), d_weights, d_z (N,S) (None = 0) -> (g_w, g_z) (N,S): g_w = d_weights + d_depth * z, g_z = d_z +
        d_depth * weights, float32 with every operation rounded on its own."""
        arr = self._arrays(weights, z_values, d_depth, d_weights, d_z)
        n, s = tuple(weights.shape)
        pw, pz = arr.inp(weights, (n, s)), arr.inp(z_values, (n, s))
        pdd = arr.inp(d_depth, (n,)) if d_depth is not None else None
        pdw = arr.inp(d_weights, (n, s)) if d_weights is not None else None
        pdz = arr.inp(d_z, (n, s)) if d_z is not None else None
        gw, pgw = arr.out((n, s))
        gz, pgz = arr.out((n, s))
        _lib.check(self.lib.nerf_render_output_grads(self.h, pw, pz, n, s, pdd, pdw, pdz, pgw, pgz, arr.mem))
        return gw, gz

    def train_render_release(self) -> None:
        """Frees the kept activations of every slot (they are grow-only otherwise; train_end frees them too)."""
        _lib.check(self.lib.nerf_train_render_release(self.h))

    def train_apply(self, grad_coarse=None, grad_fine=None) -> None:
        """Adam update from the given gradient blobs (e.g. after an all-reduce), or from the ctx's own."""
        arr = self._arrays(grad_coarse, grad_fine)
        n = self.blob_size()
        _lib.check(self.lib.nerf_train_apply(self.h, arr.inp(grad_coarse, (n,)), arr.inp(grad_fine, (n,)), arr.mem))
        self._auto_new_weights()

    def train_get_gradients(self, which: int) -> np.ndarray:
        """The gradient blob the ctx holds now (after a data-parallel ``train_step``: the all-reduced mean)."""
        out = np.empty(self.blob_size(), np.float32)
        _lib.check(self.lib.nerf_train_get_gradients(self.h, which, out.ctypes.data, out.size, NERF_MEM_HOST))
        return out

    def get_weights(self, which: int) -> np.ndarray:
        """Current weights as a flat blob in Keras ``get_weights()`` order."""
        out = np.empty(self.blob_size(), np.float32)
        _lib.check(self.lib.nerf_get_weights(self.h, which, out.ctypes.data, out.size, NERF_MEM_HOST))
        return out

    def enable_timing(self, on: bool = True) -> None:
        _lib.check(self.lib.nerf_ctx_enable_timing(self.h, int(on)))

    def read_timing(self) -> Tuple[float, int, int]:
        ms, n, rows = C.c_double(), C.c_int64(), C.c_int64()
        _lib.check(self.lib.nerf_ctx_read_timing(self.h, C.byref(ms), C.byref(n), C.byref(rows)))
        return ms.value, n.value, rows.value

    def _arrays(self, *probe) -> "_Arrays":
        """Device-resident arguments => run on torch's current stream (ordering with torch ops)."""
        arr = _Arrays(*probe)
        if arr.torch is not None:
            cur = arr.torch.cuda.current_stream(arr.device).cuda_stream
            if cur != self._stream:
                _lib.check(self.lib.nerf_ctx_set_stream(self.h, C.c_void_p(cur)))
                self._stream = cur
        return arr

    # ---- path functions ----
    def _outputs(self, arr: _Arrays, n: int, s: int, want_depth: bool, lead: Tuple[int, ...] = None):
        lead = (n,) if lead is None else lead
        rgb, p0 = arr.out(lead + (3,))
        w, p1 = arr.out(lead + (s,))
        t, p2 = arr.out(lead + (s,))
        a, p3 = arr.out(lead + (s,))
        c, p4 = arr.out(lead + (s, 3))
        z, p5 = arr.out(lead + (s,))
        d, p6 = arr.out(lead) if want_depth else (None, None)
        o = NerfOutputs(p0, p1, p2, p3, p4, p5, p6)
        return o, (rgb, w, t, a, c, z, d)

    def get_rays_directions(self, height, width, field_of_view, c2w):
        arr = self._arrays(c2w if _is_torch(c2w) else None)
        c2w_h = _host_floats(c2w, (4, 4), "c2w", exact=True)
        out, p = arr.out((height, width, 4))
        _lib.check(self.lib.nerf_get_rays_directions(self.h, c2w_h.ctypes.data, float(field_of_view), height, width,
                                                     p, arr.mem))
        return out

    def get_z_values(self, z_start, z_end, height, width, n_samples, uniform_values=None, seed=0, ray_base=0):
        """(height, width, n_samples) like src/UtilsCV.py:565-581; rays are numbered row-major."""
        if (z_start, z_end) != (self.cfg.near_boundary, self.cfg.far_boundary):
            self.set_bounds(float(z_start), float(z_end))
        arr = self._arrays(uniform_values)
        n = int(height) * int(width)
        pu = arr.inp(None if uniform_values is None else _reshape(uniform_values, (n, n_samples)), (n, n_samples))
        out, p = arr.out((height, width, n_samples))
        _lib.check(self.lib.nerf_get_z_values(self.h, n, n_samples, pu, seed, ray_base, p, arr.mem))
        return out

    def get_z_vals_from_prob_dist_func(self, weights, z_values, num_new_z_values, uniform_values=None, seed=0,
                                       ray_base=0, return_merged=False):
        arr = self._arrays(weights, z_values, uniform_values)
        n, s = tuple(weights.shape)
        pw, pz = arr.inp(weights, (n, s)), arr.inp(z_values, (n, s))
        pu = arr.inp(uniform_values, (n, num_new_z_values))
        zn, pn = arr.out((n, num_new_z_values))
        zm, pm = arr.out((n, s + num_new_z_values)) if return_merged else (None, None)
        _lib.check(self.lib.nerf_sample_pdf(self.h, pw, pz, n, s, num_new_z_values, pu, seed, ray_base, pn, pm,
                                            arr.mem))
        return (zn, zm) if return_merged else zn

    def positional_encoding(self, x, n_positional_encoding, passthrough):
        arr = self._arrays(x)
        m = int(x.shape[0])
        px = arr.inp(x, (m, 3))
        per = 3 * ((1 if passthrough else 0) + 2 * n_positional_encoding)
        out, p = arr.out((m, per))
        _lib.check(self.lib.nerf_positional_encoding(self.h, px, m, n_positional_encoding, int(passthrough), p,
                                                     arr.mem))
        return out

    def model_predict(self, which, xyz, view_dirs):
        arr = self._arrays(xyz, view_dirs)
        m = int(xyz.shape[0])
        if self.cfg.n_angles == 0:                      # xyz-only network: no direction input (UtilsNRF.py:229-234)
            def run0():
                out, p = arr.out((m, 4))
                _lib.check(self.lib.nerf_model_predict(self.h, which, arr.inp(xyz, (m, 3)), None, m, p, arr.mem))
                return out
            return self._auto_call(run0, arr.mem)
        if self.cfg.n_angles == 1 and tuple(view_dirs.shape) == (m, 2):
            # the reference hands (x, z) to the n_angles == 1 network (src/UtilsCV.py:134-135); the
            # library takes full directions and ignores y through zero-packed weights
            if arr.torch is not None and _is_torch(view_dirs):
                z0 = arr.torch.zeros_like(view_dirs[:, :1])
                view_dirs = arr.torch.cat([view_dirs[:, :1], z0, view_dirs[:, 1:]], dim=1)
            else:
                v = np.asarray(view_dirs, np.float32)
                view_dirs = np.stack([v[:, 0], np.zeros(m, np.float32), v[:, 1]], axis=1)
        px, pv = arr.inp(xyz, (m, 3)), arr.inp(view_dirs, (m, 3))

        def run():
            out, p = arr.out((m, 4))
            _lib.check(self.lib.nerf_model_predict(self.h, which, px, pv, m, p, arr.mem))
            return out
        return self._auto_call(run, arr.mem)

    def ray_marching(self, model_output, z_values):
        arr = self._arrays(model_output, z_values)
        n, s = tuple(z_values.shape)
        pr, pz = arr.inp(model_output, (n, s, 4)), arr.inp(z_values, (n, s))
        o, res = self._outputs(arr, n, s, False)
        o.z = None
        _lib.check(self.lib.nerf_ray_marching(self.h, pr, pz, n, s, C.byref(o), arr.mem))
        return res[:5]

    def render_rays(self, which, rays_orig, rays_dirs, z_values):
        arr = self._arrays(rays_orig, rays_dirs, z_values)
        n, s = tuple(z_values.shape)
        po, pd, pz = arr.inp(rays_orig, (n, 4)), arr.inp(rays_dirs, (n, 4)), arr.inp(z_values, (n, s))

        def run():
            o, res = self._outputs(arr, n, s, False)
            o.z = None
            _lib.check(self.lib.nerf_render_rays(self.h, which, po, pd, pz, n, s, C.byref(o), arr.mem))
            return res[:5]
        return self._auto_call(run, arr.mem)

    def render(self, rays_orig, rays_dirs, n_c, n_f, u_coarse=None, u_fine=None, seed=0, ray_base=0,
               want_depth=False):
        arr = self._arrays(rays_orig, rays_dirs, u_coarse, u_fine)
        n = int(rays_orig.shape[0])
        fine = n_f > 0 and self.loaded[NERF_NET_FINE]
        s = n_c + n_f if fine else n_c
        po, pd = arr.inp(rays_orig, (n, 4)), arr.inp(rays_dirs, (n, 4))
        puc = arr.inp(u_coarse, (n, n_c))
        puf = arr.inp(u_fine, (n, n_f)) if fine else None

        def run():
            o, res = self._outputs(arr, n, s, want_depth)
            _lib.check(self.lib.nerf_render(self.h, po, pd, n, n_c, n_f if fine else 0, puc, puf, seed, ray_base,
                                            C.byref(o), arr.mem))
            return res if want_depth else res[:6]
        return self._auto_call(run, arr.mem)

    def render_image(self, c2w, fov, h, w, batch, n_c, n_f, u_coarse=None, u_fine=None, seed=0, ray_begin=0,
                     ray_count=0, want_depth=False, device_out=False, rgb_only=False):
        """Whole image (ray_count=0) -> outputs shaped (h,w,...); a slab -> outputs shaped (ray_count,...)."""
        arr = self._arrays(u_coarse, u_fine)
        if device_out and arr.torch is None:
            import torch
            arr = self._arrays(torch.empty(1, device=torch.device("cuda", self.cfg.device)))
        c2w_h = _host_floats(c2w, (4, 4), "c2w", exact=True)
        total = h * w
        fine = n_f > 0 and self.loaded[NERF_NET_FINE]
        s = n_c + n_f if fine else n_c
        puc = arr.inp(u_coarse, (total, n_c))
        puf = arr.inp(u_fine, (total, n_f)) if fine else None
        whole = ray_count <= 0
        n = total if whole else ray_count
        lead = (h, w) if whole else (n,)

        def run():
            if rgb_only:
                rgb, p0 = arr.out(lead + (3,))
                d, p6 = arr.out(lead) if want_depth else (None, None)
                o, res = NerfOutputs(p0, None, None, None, None, None, p6), (rgb, None, None, None, None, None, d)
            else:
                o, res = self._outputs(arr, n, s, want_depth, lead)
            _lib.check(self.lib.nerf_render_image(self.h, c2w_h.ctypes.data, float(fov), h, w, 0 if whole else ray_begin,
                                                  0 if whole else ray_count, batch or 0, n_c, n_f if fine else 0, puc,
                                                  puf, seed, C.byref(o), arr.mem))
            return res if want_depth else res[:6]
        return self._auto_call(run, arr.mem)


def _metrics(m, fine: bool) -> Dict[str, float]:
    out = {"loss": float(m[0]), "psnr_coarse": float(m[1])}
    if fine:
        out["psnr_fine"] = float(m[2])
    return out


def _reshape(x, shape):
    return x.reshape(shape)


class NetHandle:
    """Stands in for the Keras ``model`` argument of render_rays / model_predict."""

    def __init__(self, ctx: Context, which: int):
        self.ctx, self.which = ctx, which


class NeRF:
    """Mirror of the reference model class (src/NeRF.py:22-246): render path and train_step.

    ``precision`` is the render path's arithmetic (``Context``): "auto" (default), "fp32", "f16x3", "bf16x3" (3-pass
    split-bf16 MFMA: fp32-class results with fp32's exponent range) or "f16".  train_step does not depend on it."""

    def __init__(self, net_config: Dict, render_config: Dict, near_boundary: float, far_boundary: float,
                 device: int = 0, precision: str = "auto"):
        self.ctx = Context(n_pos_enc_xyz=net_config[N_POS_ENC_DIM_XYZ], n_pos_enc_dir=net_config[N_POS_ENC_VIEW_DIR],
                           n_angles=net_config[N_ANGLES_FOR_MODEL], hidden_dim=net_config[HIDDEN_LAYER_DIM],
                           last_hidden_dim=net_config[LAST_HIDDEN_LAYER_DIM],
                           leaky_relu_alpha=net_config[LEAKY_RELU_ALPHA], near=near_boundary, far=far_boundary,
                           precision=precision, device=device)
        self.model_coarse = NetHandle(self.ctx, NERF_NET_COARSE)
        self.model_fine = NetHandle(self.ctx, NERF_NET_FINE) if render_config[N_RENDER_SAMPLES_FINE] > 0 else None
        self.batch_size_render = net_config.get(N_RAYS_IN_BATCH_RENDER, 4096)
        self.batch_size_train = net_config.get(N_RAYS_IN_BATCH_TRAIN, 4096)
        self.near_boundary, self.far_boundary = near_boundary, far_boundary
        self.n_render_samples_coarse = render_config[N_RENDER_SAMPLES_COARSE]
        self.n_render_samples_fine = render_config[N_RENDER_SAMPLES_FINE]
        self.n_pos_enc_dim_xyz = net_config[N_POS_ENC_DIM_XYZ]
        self.n_pos_enc_view_dir = net_config[N_POS_ENC_VIEW_DIR]
        self.n_angles_for_model = net_config[N_ANGLES_FOR_MODEL]
        self.seed = 0
        # forward-facing scenes: absent keys leave the context as nerf_ctx_create made it (linear depths, world rays)
        self.lindisp = bool(render_config.get(LINDISP, False))
        self.use_ndc = bool(render_config.get(USE_NDC, False))
        self.ndc_near_plane = float(render_config.get(NDC_NEAR_PLANE, 1.0))
        if self.lindisp:
            self.ctx.set_sampling("lindisp")
        if self.use_ndc:
            self.ctx.set_ray_space("ndc", self.ndc_near_plane)
        # scene box: an absent key (or None) leaves the context without one
        self.scene_box = render_config.get(SCENE_BOX)
        if self.scene_box is not None:
            if len(self.scene_box) != 2:
                raise ValueError(f"{SCENE_BOX} must be [[x, y, z], [x, y, z]] (lo, hi), got {self.scene_box!r}")
            self.ctx.set_scene_box(self.scene_box[0], self.scene_box[1])
        # occupancy grid: an absent key (or None) leaves everything as it was
        self.grid_config = self._grid_config(render_config.get(OCCUPANCY_GRID), self.scene_box)
        self._grid_epochs = 0        # epochs fit() has run: the grid's schedule counts them
        self._preview = None         # bake_preview: (volume on the device, lo, hi, resolution)
        self._preview_sh_degree = None     # ... and the SH degree of that volume (None: the plain RGB-sigma volume)
        if self.grid_config is not None and self.grid_config.get(GRID_CULL_SAMPLES, False):
            self.ctx.set_sample_culling(True)
        if self.grid_config is not None and self.grid_config.get(GRID_CULL_TRAIN_SAMPLES, False):
            self.ctx.set_train_sample_culling(True)
        # distortion regulariser: an absent key leaves training as it was; compile() hands the weights to the trainer
        self.distortion_weights = check_distortion_loss(render_config[DISTORTION_LOSS]) if DISTORTION_LOSS in render_config \
            else None
        # coarse-to-fine encoding: an absent key leaves everything as it was; compile() applies epoch 0, fit() the rest
        self.window_config = check_encoding_window(render_config[ENCODING_WINDOW], self.n_pos_enc_dim_xyz) \
            if ENCODING_WINDOW in render_config else None
        self._window_epochs = 0      # epochs fit() has run since compile(): the window's schedule counts them

    @staticmethod
    def _grid_config(cfg, scene_box):
        """render_config["occupancy_grid"] checked and completed with its defaults, or None."""
        if cfg is None:
            return None
        if scene_box is None:
            raise ValueError(f"{OCCUPANCY_GRID}: {GRID_NEEDS_BOX} (render_config[{SCENE_BOX!r}])")
        unknown = sorted(set(cfg) - set(_GRID_KEYS))
        if unknown:
            raise ValueError(f"{OCCUPANCY_GRID}: unknown keys {unknown}; expected {list(_GRID_KEYS)}")
        for key in (GRID_RESOLUTION, GRID_SIGMA_THRESHOLD):
            if key not in cfg:
                raise ValueError(f"{OCCUPANCY_GRID} needs {key!r}")
        out = {GRID_RESOLUTION: check_grid_resolution(cfg[GRID_RESOLUTION]), GRID_SIGMA_THRESHOLD: float(cfg[GRID_SIGMA_THRESHOLD]),
               GRID_SAMPLES_PER_CELL: int(cfg.get(GRID_SAMPLES_PER_CELL, 1)), GRID_DILATE: int(cfg.get(GRID_DILATE, 1)),
               GRID_UPDATE_EVERY: int(cfg.get(GRID_UPDATE_EVERY, 1)), GRID_WARMUP_EPOCHS: int(cfg.get(GRID_WARMUP_EPOCHS, 0))}
        if not (np.isfinite(out[GRID_SIGMA_THRESHOLD]) and out[GRID_SIGMA_THRESHOLD] > 0):
            raise ValueError(f"{OCCUPANCY_GRID}: sigma_threshold must be finite and > 0 (got {cfg[GRID_SIGMA_THRESHOLD]!r})")
        if not 1 <= out[GRID_SAMPLES_PER_CELL] <= 8:
            raise ValueError(f"{OCCUPANCY_GRID}: samples_per_cell must be in 1..8 (got {cfg[GRID_SAMPLES_PER_CELL]!r})")
        if out[GRID_DILATE] not in (0, 1, 2):
            raise ValueError(f"{OCCUPANCY_GRID}: dilate must be 0, 1 or 2 (got {cfg[GRID_DILATE]!r})")
        if out[GRID_UPDATE_EVERY] < 1 or out[GRID_WARMUP_EPOCHS] < 0:
            raise ValueError(f"{OCCUPANCY_GRID}: update_every must be >= 1 and warmup_epochs >= 0")
        if GRID_CULL_SAMPLES in cfg:       # without the key the config is what it was
            if not isinstance(cfg[GRID_CULL_SAMPLES], (bool, np.bool_)):
                raise ValueError(f"{OCCUPANCY_GRID}: {GRID_CULL_SAMPLES} must be a bool (got {cfg[GRID_CULL_SAMPLES]!r})")
            out[GRID_CULL_SAMPLES] = bool(cfg[GRID_CULL_SAMPLES])
        if GRID_CULL_TRAIN_SAMPLES in cfg:
            if not isinstance(cfg[GRID_CULL_TRAIN_SAMPLES], (bool, np.bool_)):
                raise ValueError(f"{OCCUPANCY_GRID}: {GRID_CULL_TRAIN_SAMPLES} must be a bool (got {cfg[GRID_CULL_TRAIN_SAMPLES]!r})")
            out[GRID_CULL_TRAIN_SAMPLES] = bool(cfg[GRID_CULL_TRAIN_SAMPLES])
        return out

    def update_occupancy_grid(self, seed: int = 0) -> Optional[int]:
        """Bake the configured grid (render_config["occupancy_grid"]) from the fine network when it is loaded, otherwise the
        coarse one; returns the occupied count, or None without the key.  load_weights calls it, and dataset.fit calls it
        every ``update_every`` epochs once ``warmup_epochs`` have passed (before that the grid is off).  Nowhere else is the
        grid rebuilt: after set_weights or train_step calls of the caller's own it is stale until this is called again, and
        training with a stale grid is the caller's choice."""
        g = self.grid_config
        if g is None:
            return None
        which = NERF_NET_FINE if self.model_fine is not None and self.ctx.loaded[NERF_NET_FINE] else NERF_NET_COARSE
        return self.ctx.bake_occupancy_grid(which, g[GRID_RESOLUTION], g[GRID_SIGMA_THRESHOLD], g[GRID_SAMPLES_PER_CELL],
                                            g[GRID_DILATE], seed)

    def extract_mesh(self, resolution: int = 128, sigma_threshold: float = 50.0, which: Optional[int] = None, colors: bool = True,
                     path=None) -> Dict[str, np.ndarray]:
        """The scene as a triangle mesh: the density of network ``which`` (None: the fine network if it is loaded, else the
        coarse one) on a ``resolution``^3 lattice over render_config["scene_box"], its isosurface at ``sigma_threshold``
        (raw sigma, the unit of the occupancy grid's threshold), and per-vertex colours seen against the normals.  Returns
        numpy arrays: "vertices" (V, 3) float32, "normals" (V, 3) float32 (unit, pointing out of the density; zero where the
        gradient vanishes), "triangles" (T, 3) int32 (counter-clockwise from outside) and, with ``colors``, "colors" (V, 3)
        float32 in [0, 1].  ``path``: also write a binary little-endian PLY there (mesh.write_ply).  The mesh is closed
        except where the surface leaves the box."""
        if self.scene_box is None:
            raise ValueError(f"extract_mesh needs render_config[{SCENE_BOX!r}]")
        if which is None:
            which = NERF_NET_FINE if self.model_fine is not None and self.ctx.loaded[NERF_NET_FINE] else NERF_NET_COARSE
        try:
            import torch
            on_device = torch.cuda.is_available()
        except ImportError:
            on_device = False
        sigma = self.ctx.density_lattice(which, resolution, device_out=on_device)      # the volume stays on the device
        vertices, triangles, normals = self.ctx.isosurface(sigma, self.scene_box[0], self.scene_box[1], sigma_threshold)
        rgb = self.ctx.mesh_colors(which, vertices, normals) if colors else None
        if on_device and self.ctx.auto_check():          # precision "auto": the f16x3 pass overflowed, the context is in fp32 now
            return self.extract_mesh(resolution, sigma_threshold, which, colors, path)
        host = (lambda x: x.cpu().numpy()) if on_device else (lambda x: x)
        mesh = {"vertices": host(vertices), "normals": host(normals), "triangles": host(triangles)}
        if colors:
            mesh["colors"] = host(rgb)
        if path is not None:
            from .mesh import write_ply
            write_ply(path, mesh["vertices"], mesh["triangles"], mesh["normals"], mesh.get("colors"))
        return mesh

    def bake_preview(self, resolution: int = 256, which: Optional[int] = None, view_dir=None, camera=None, sh_degree=None,
                     sh_dirs=None, sh_proj=None) -> None:
        """Bake network ``which`` (None: the fine network if it is loaded, else the coarse one) onto a ``resolution``^3
        RGB-sigma lattice over render_config["scene_box"] (Context.radiance_lattice) and keep it, as a device tensor together
        with the box it was baked on, for render_preview.  Colours are those of ONE view direction (``view_dir``, default
        (0, 0, 1)) or ONE camera (``camera``, a (4, 4) camera-to-world matrix): the preview shows no view-dependent effects
        from any other pose and is no parity mode of render_image.  It is a snapshot, like the occupancy grid: nothing
        rebuilds it -- training on, loading other weights or changing the box leave it as baked until this is called again.
        16 bytes a vertex: 256 MiB at 256, 2 GiB at 512.

        ``sh_degree`` (0..3): bake view-dependent colour instead, as spherical harmonics of that degree per vertex
        (Context.sh_radiance_lattice; ``sh_dirs`` / ``sh_proj``: a projection table other than the default full-sphere one).
        One bake then serves every pose, for the unit view direction; it cannot be combined with ``view_dir`` or ``camera``,
        and a vertex takes 16 / 64 / 112 / 208 bytes."""
        if self.scene_box is None:
            raise ValueError(f"bake_preview needs render_config[{SCENE_BOX!r}]")
        if sh_degree is None:
            if sh_dirs is not None or sh_proj is not None:
                raise ValueError("bake_preview: sh_dirs and sh_proj need sh_degree")

            def bake():
                return self.ctx.radiance_lattice(which, resolution, view_dir=view_dir, camera=camera, device_out=True)
        else:
            if view_dir is not None or camera is not None:
                raise ValueError("bake_preview: sh_degree cannot be combined with view_dir or camera")
            sh_degree = check_sh_degree(sh_degree)

            def bake():
                return self.ctx.sh_radiance_lattice(which, resolution, sh_degree, dirs=sh_dirs, proj=sh_proj, device_out=True)
        if which is None:
            which = NERF_NET_FINE if self.model_fine is not None and self.ctx.loaded[NERF_NET_FINE] else NERF_NET_COARSE
        self._preview = None
        self._preview_sh_degree = None
        volume = bake()
        if self.ctx.auto_check():            # precision "auto": the f16x3 pass overflowed, the context is in fp32 now
            volume = bake()
        self._preview = (volume, tuple(self.scene_box[0]), tuple(self.scene_box[1]), int(resolution))
        self._preview_sh_degree = sh_degree

    def render_preview(self, c2w, fov, h, w, n_steps: Optional[int] = None, t_min: float = 1.0 / 512.0):
        """The baked preview seen from camera ``c2w``: (rgb (h, w, 3), depth (h, w), opacity (h, w)) as torch-device
        tensors, by marching the volume of bake_preview in ``n_steps`` steps per ray (default 2 * resolution) with no network
        in the loop (Context.render_volume_image).  rgb is premultiplied by opacity.  depth is a depth MAP: the mean depth of
        what the ray met, the march's weighted sum of step depths over its opacity -- inside the ray's stretch of [near, far]
        whatever the opacity, where the sum itself shrinks with it -- and 0 where the ray met nothing (opacity 0); it means
        little where the opacity is tiny.  ``t_min``: a ray stops once its transmittance is below it; the default 1/512 keeps
        the error under half an 8-bit level.  The preview is as baked: see bake_preview for what it is not."""
        if self._preview is None:
            raise RuntimeError("render_preview: no preview is baked (call bake_preview first)")
        volume, lo, hi, resolution = self._preview
        march = self.ctx.render_volume_image if self._preview_sh_degree is None else self.ctx.render_sh_volume_image
        rgb, depth_sum, opacity = march(volume, lo, hi, c2w, fov, h, w, 2 * resolution if n_steps is None else n_steps, t_min)
        depth = depth_sum.div_(opacity).masked_fill_(opacity <= 0, 0.0)      # on the device, no synchronisation
        return rgb, depth, opacity

    def occupancy_grid_epoch(self) -> None:
        """dataset.fit's hook, at the start of every epoch: the grid is off during the warm-up epochs and baked again every
        ``update_every`` epochs after them."""
        g = self.grid_config
        if g is None:
            return
        done = self._grid_epochs - g[GRID_WARMUP_EPOCHS]
        self._grid_epochs += 1
        if done < 0:
            if self.ctx.grid_resolution:
                self.ctx.set_occupancy_grid(None)
        elif done % g[GRID_UPDATE_EVERY] == 0:
            self.update_occupancy_grid()

    # ---- coarse-to-fine positional encoding (Context.set_encoding_window) ----
    def set_encoding_alpha(self, alpha_xyz, alpha_dirs=None, kind: str = "cosine") -> None:
        """Open the xyz encoding's window to progress ``alpha_xyz`` in [0, n_pos_enc_dim_xyz] (``encoding_window``) and, with
        ``alpha_dirs``, the direction encoding's to that one in [0, n_pos_enc_view_dir]; None leaves the directions at full
        band.  Per-step control for a caller's own loop -- a pose refinement that opens the window as it converges.  At
        alpha_xyz >= n_pos_enc_dim_xyz (and no direction window) the window is off."""
        wx = encoding_window(alpha_xyz, self.n_pos_enc_dim_xyz, kind)
        wd = None if alpha_dirs is None else encoding_window(alpha_dirs, self.n_pos_enc_view_dir, kind)
        self.ctx.set_encoding_window(wx, wd)

    def encoding_window_epoch(self) -> None:
        """dataset.fit's hook, at the start of every epoch and before the occupancy grid's (a re-baked grid sees the epoch's
        window): with render_config["encoding_window"] = {"kind", "start", "end", "epochs", "dirs"} epoch e, counted from
        compile(), trains under alpha_xyz = start + (end - start) min(e / epochs, 1); with "dirs" the direction encoding
        gets alpha_xyz * n_pos_enc_view_dir / n_pos_enc_dim_xyz.  Once alpha reaches n_pos_enc_dim_xyz the window is off and
        a checkpoint saved from then on is an ordinary network.  A checkpoint saved mid-schedule does NOT record the window:
        it holds the master weights, which render as trained only under the window of that epoch."""
        w = self.window_config
        if w is None:
            return
        alpha = encoding_window_alpha(w, self._window_epochs)
        self._window_epochs += 1
        self.set_encoding_alpha(alpha, alpha * self.n_pos_enc_view_dir / self.n_pos_enc_dim_xyz if w[WINDOW_DIRS] else None,
                                w[WINDOW_KIND])

    def set_weights(self, coarse, fine=None) -> None:
        self._blobs = [coarse, fine]
        self.ctx.load_weights(NERF_NET_COARSE, coarse)
        if fine is not None and self.model_fine is not None:
            self.ctx.load_weights(NERF_NET_FINE, fine)

    def load_weights(self, path) -> None:
        """Keras ``model.load_weights(path)`` for the reference's ``NeRF_model_epoch_XXX.h5`` files
        (src/ExecutionRun.py:228-231) -- parsed by the built-in pure-Python HDF5 reader."""
        from .keras_h5 import load_nerf_checkpoint
        coarse, fine = load_nerf_checkpoint(str(path))
        self.set_weights(coarse, fine)
        self.update_occupancy_grid()     # render_config["occupancy_grid"]: a loaded checkpoint is rendered with its own grid

    def save_weights(self, path) -> None:
        """Keras ``model.save_weights(path)`` (src/UtilsFiles.py:153-164): the current (trained) weights as a
        Keras-2.7 style ``.h5`` that h5py / the reference's ``model.load_weights`` read."""
        from .keras_h5 import save_nerf_checkpoint
        coarse, fine = self.get_weights()
        save_nerf_checkpoint(str(path), coarse, fine, n_pos_enc_xyz=self.n_pos_enc_dim_xyz,
                             n_pos_enc_dir=self.n_pos_enc_view_dir, n_angles=self.n_angles_for_model)

    @staticmethod
    def get_nerf_model_path(save_location, epoch_number: int):
        """src/NeRF.py:342-351."""
        from pathlib import Path
        return Path(save_location) / "saved_weights" / "NeRF_model_epoch_{:03}.h5".format(epoch_number)

    # ---- training: model.compile(optimizer=Adam(lr)) + train_step (src/ExecutionRun.py:226-227, src/NeRF.py:136-178)
    def compile(self, optimizer_lr: float, beta_1: float = 0.9, beta_2: float = 0.999, epsilon: float = 1e-7,
                sampler_gradient: bool = True, mixed_float16: bool = False, initial_loss_scale: float = 0.0,
                dynamic_growth_steps: int = 0) -> None:
        self.ctx.train_begin(optimizer_lr, beta_1, beta_2, epsilon, sampler_gradient, mixed_float16, initial_loss_scale,
                             dynamic_growth_steps)
        self._train_calls = 0
        self._mixed = bool(mixed_float16)
        if self.distortion_weights is not None:
            self.ctx.train_set_distortion_weights(*self.distortion_weights)
        if getattr(self, "window_config", None) is not None:      # the schedule starts over: epoch 0's window, now
            self._window_epochs = 0
            self.encoding_window_epoch()
            self._window_epochs = 0

    def train_read_extra_metric_sums(self):
        """Sums of the two distortion losses over the steps since the last read, for dataset.fit's per-epoch means -- only
        with a non-zero render_config["distortion_loss"], so the histories of other runs keep their keys.
        -> ({"distortion_coarse", "distortion_fine"}: sums, steps)"""
        weights = getattr(self, "distortion_weights", None)
        if not (weights and any(weights)):
            return {}, 0
        return self.ctx.train_read_distortion_sums()

    def train_step(self, data, *, u_coarse=None, u_fine=None, seed=None, group=None,
                   want_metrics: bool = True) -> Optional[Dict[str, float]]:
        """``data`` = (rays_orig (N,4), rays_dirs (N,4), real_rgb (N,3)) -> {"loss", "psnr_coarse"[, "psnr_fine"]}.
        ``want_metrics=False`` does not wait for the step (the metrics still enter the device-side sums that
        ``ctx.train_read_metric_sums()`` hands out: dataset.fit reads them once per epoch).

        Under an initialised torch.distributed ``group`` every rank passes its own shard of the batch; the
        gradient blobs are averaged with one all-reduce each before the identical Adam update: inside the library
        (ncclAllReduce on the ctx stream) when the ctx has joined a communicator of the group's size
        (``ctx.comm_init_from_torch(group)``), otherwise through the group itself (RCCL under nccl; gloo stages through the
        host).  Under mixed_float16 both ways test the REDUCED blobs, so every rank skips the same steps and moves its loss
        scale alike (src/NeRF.py:159-163 on each replica)."""
        rays_orig, rays_dirs, real_rgb = data
        n_f = self.n_render_samples_fine if self.model_fine else 0
        if seed is None:
            seed = self.seed + 7919 * self._train_calls
        self._train_calls += 1
        from .sharding import dist_world
        world = dist_world(group)
        if world == 1 or self.ctx.comm_world == world:
            return self.ctx.train_step(rays_orig, rays_dirs, real_rgb, self.n_render_samples_coarse, n_f, u_coarse,
                                       u_fine, seed, want_metrics)
        if self.ctx.comm_world:
            raise RuntimeError(f"the context's communicator has {self.ctx.comm_world} ranks, the group {world}")
        from .sharding import allreduce_mean
        metrics, gc, gf = self.ctx.train_gradients(rays_orig, rays_dirs, real_rgb, self.n_render_samples_coarse, n_f,
                                                   u_coarse, u_fine, seed)
        gc = allreduce_mean(gc, group, self.ctx.cfg.device)
        gf = allreduce_mean(gf, group, self.ctx.cfg.device) if gf is not None else None
        self.ctx.train_apply(gc, gf)
        return metrics if want_metrics else None

    def train_step_custom(self, batch, loss_fn, slot: int = 0, *, u_coarse=None, u_fine=None, seed=None,
                          want_loss: bool = False) -> Optional[float]:
        """One optimizer step on a loss written in torch: ``batch`` = (rays_orig (N,4), rays_dirs (N,4), real_rgb) as torch
        device tensors; ``loss = loss_fn(outputs, real_rgb)`` with ``outputs`` the dict of ``autograd.render_with_grad``
        (rgb, depth, weights, z of ``render()`` on these rays); then ``loss.backward()`` and the Adam update.  Returns
        ``float(loss)`` only with ``want_loss=True`` (which waits for the step), else None.  Under mixed_float16 do NOT scale
        the loss: the library multiplies the cotangents by its loss scale on the device, unscales the gradients and skips a
        non-finite step.  Single process only (no ``group``)."""
        from .autograd import render_with_grad
        rays_orig, rays_dirs, real_rgb = batch
        n_f = self.n_render_samples_fine if self.model_fine else 0
        if seed is None:
            seed = self.seed + 7919 * self._train_calls
        self._train_calls += 1
        out = render_with_grad(self.ctx, rays_orig, rays_dirs, self.n_render_samples_coarse, n_f, slot=slot, seed=seed,
                               u_coarse=u_coarse, u_fine=u_fine)
        loss = loss_fn(out, real_rgb)
        loss.backward()
        self.ctx.train_apply()
        return float(loss.detach()) if want_loss else None

    def get_weights(self):
        """(coarse blob, fine blob | None), Keras ``get_weights()`` order."""
        return (self.ctx.get_weights(NERF_NET_COARSE),
                self.ctx.get_weights(NERF_NET_FINE) if self.model_fine and self.ctx.loaded[1] else None)

    def call(self, inputs, training=None, mask=None):
        rays_orig, rays_dirs = inputs
        return self.render(rays_orig, rays_dirs)[0]

    __call__ = call

    def render(self, rays_orig, rays_dirs, n_render_samples_c=None, n_render_samples_f=None, *, u_coarse=None,
               u_fine=None, seed=None, ray_base=0):
        n_c = n_render_samples_c if n_render_samples_c else self.n_render_samples_coarse
        n_f = 0
        if self.model_fine:
            n_f = n_render_samples_f if n_render_samples_f else self.n_render_samples_fine
        return self.ctx.render(rays_orig, rays_dirs, n_c, n_f, u_coarse, u_fine,
                               self.seed if seed is None else seed, ray_base)

    def render_rays(self, model: NetHandle, rays_orig, rays_dirs, z):
        return render_rays(model, rays_orig, rays_dirs, z, self.n_pos_enc_dim_xyz, self.n_pos_enc_view_dir,
                           self.n_angles_for_model)

    def render_image(self, c2w, fov, h, w, batch_size_input=None, n_render_samples_c=None, n_render_samples_f=None,
                     *, u_coarse=None, u_fine=None, seed=None, **kw):
        batch = batch_size_input if batch_size_input else self.batch_size_render
        assert batch > 0                                           # src/UtilsNRF.py:25
        # The reference's render batch (4096 / 16384 rays) bounds TensorFlow's activation memory; here nothing per-layer
        # is materialised and results do not depend on the batch (tests/test_gpu_parity.py::test_full_size_properties),
        # so the library's own batch is used unless the caller insists (``honor_batch=True``).
        if not kw.pop("honor_batch", False):
            batch = 0
        n_c = n_render_samples_c if n_render_samples_c else self.n_render_samples_coarse
        n_f = 0
        if self.model_fine:
            n_f = n_render_samples_f if n_render_samples_f else self.n_render_samples_fine
        return self.ctx.render_image(c2w, fov, h, w, batch, n_c, n_f, u_coarse, u_fine,
                                     self.seed if seed is None else seed, **kw)


# --------------------------------------------------------------------------------------------
# free functions with the reference's signatures
# --------------------------------------------------------------------------------------------
_default_ctx: Optional[Context] = None


def default_context() -> Context:
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context()
    return _default_ctx


def render_rays(model: NetHandle, rays_orig, rays_dirs, z_values, n_pos_enc_for_xyz: int, n_pos_enc_for_angles: int,
                n_angles_for_model: int):
    """src/UtilsNeuralRadianceField.py:181-211 -> (render_result, weights, cumprod, alpha, rgb)."""
    cfg = model.ctx.cfg
    if n_angles_for_model not in (0, 1, 2):    # 0: render_rays never calls get_view_directions (UtilsNRF.py:205)
        raise Exception(f"{N_ANGLES_FOR_MODEL} should be 1 or 2.")   # src/UtilsCV.py:138
    if (n_pos_enc_for_xyz, n_pos_enc_for_angles, n_angles_for_model) != (cfg.n_pos_enc_xyz, cfg.n_pos_enc_dir,
                                                                         cfg.n_angles):
        raise ValueError("encoding arguments do not match the network this model handle was built with")
    return model.ctx.render_rays(model.which, rays_orig, rays_dirs, z_values)


def model_predict(model: NetHandle, n_enc_phi_theta: int, n_pos_enc_for_xyz: int, xyz, view_dirs=None):
    """src/UtilsNeuralRadianceField.py:214-234 -> (M,4) raw (R,G,B,Sigma)."""
    cfg = model.ctx.cfg
    # the encodings are the network's (its layer shapes follow them): counts that differ from it are a caller error
    # (the xyz-only network has no direction input: n_enc_phi_theta is not used by it, src/UtilsNeuralRadianceField.py:229-234)
    if n_pos_enc_for_xyz != cfg.n_pos_enc_xyz or (cfg.n_angles != 0 and n_enc_phi_theta != cfg.n_pos_enc_dir):
        raise ValueError("encoding arguments do not match the network this model handle was built with")
    if view_dirs is None and model.ctx.cfg.n_angles != 0:
        raise ValueError("view_dirs is None but this model takes view directions")
    return model.ctx.model_predict(model.which, xyz, view_dirs)


def ray_marching(model_output, z_values, ctx: Optional[Context] = None):
    """src/UtilsNeuralRadianceField.py:88-115."""
    return (ctx or default_context()).ray_marching(model_output, z_values)


def positional_encoding_for_xyz(xyz, n_positional_encoding: int, ctx: Optional[Context] = None):
    """src/UtilsNeuralRadianceField.py:68-85."""
    if n_positional_encoding == 0:
        return xyz.reshape(xyz.shape[0], -1)
    return (ctx or default_context()).positional_encoding(xyz, n_positional_encoding, True)


def positional_encoding_for_views(x, n_positional_encoding: int, ctx: Optional[Context] = None):
    """src/UtilsNeuralRadianceField.py:52-65 (3-component view directions)."""
    return (ctx or default_context()).positional_encoding(x, n_positional_encoding, False)


def get_rays_directions(height, width, field_of_view, c2w, ctx: Optional[Context] = None):
    """src/UtilsCV.py:467-499 -> (H,W,4)."""
    return (ctx or default_context()).get_rays_directions(height, width, field_of_view, c2w)


def get_z_values(z_start, z_end, height, width, n_samples, uniform_values=None, seed=0,
                 ctx: Optional[Context] = None):
    """src/UtilsCV.py:565-581 -> (height, width, n_samples)."""
    return (ctx or default_context()).get_z_values(z_start, z_end, height, width, n_samples, uniform_values, seed)


def get_z_vals_from_prob_dist_func(weights, z_values, num_new_z_values, uniform_values=None, seed=0,
                                   ctx: Optional[Context] = None):
    """src/UtilsCV.py:502-539 -> sorted (N, num_new_z_values)."""
    return (ctx or default_context()).get_z_vals_from_prob_dist_func(weights, z_values, num_new_z_values,
                                                                   uniform_values, seed)


def get_size_of_splits(batch_size: int, total_size: int) -> List[int]:
    """src/UtilsNeuralRadianceField.py:32-49 (host logic: defines launch granularity only)."""
    n_full_batches = total_size // batch_size
    if n_full_batches == 0:
        return [total_size]
    if total_size % batch_size != 0:
        return [batch_size] * n_full_batches + [-1]
    return [batch_size] * n_full_batches


def split_to_batches(to_split, batch_size):
    """src/UtilsNeuralRadianceField.py:17-29."""
    assert batch_size > 0
    total = to_split.shape[0]
    out, off = [], 0
    for s in get_size_of_splits(batch_size, total):
        s = total - off if s == -1 else s
        out.append(to_split[off:off + s])
        off += s
    return out
