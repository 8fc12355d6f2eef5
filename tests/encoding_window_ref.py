"""Reference of the encoding window (include/nerf_mi355.h: nerf_ctx_set_encoding_window) -- TEST INFRASTRUCTURE ONLY.

Written from the rule the window is specified by, not from the library's tables:

    the blob is, layer by layer, kernel (in, out) row-major then bias;
    layer 0's input is the xyz encoding, per component c: [x_c, sin_0, cos_0, ..., sin_(L-1), cos_(L-1)]  (1 + 2 L rows);
    layer 4's input is [xyz encoding (3 + 6 L rows) | hidden (256)];
    with view directions (n_angles 1 or 2) the input of layers 8 and 10 is [hidden (256) | direction encoding], per
    component c < n_angles + 1: [sin_0, cos_0, ..., sin_(Ld-1), cos_(Ld-1)]  (2 Ld rows);
    S = w_xyz[k] on the rows of octave k of the xyz encoding, w_dir[k] on those of the direction encoding, 1 elsewhere.

    scale_table(L, Ld, n_angles, w_xyz, w_dir) -> S, float32, one value per blob element
    fold(blob, S)                              -> fl32(blob * S)
    cosine_window / linear_window(alpha, n)    -> the two schedules' per-octave weights (float64)
    masks(L, Ld, n_angles, w_xyz, w_dir)       -> the per-feature factors of the two encodings themselves
"""
import numpy as np

HIDDEN, LAST = 256, 128


def layer_shapes(L, Ld, n_angles):
    """[(rows, cols)] of every kernel, in blob order (src/NeRF.py:248-288, 312-337)."""
    xd, dd = 3 + 6 * L, 2 * Ld * (n_angles + 1)
    trunk = [(xd, HIDDEN)] + [(HIDDEN, HIDDEN)] * 3 + [(xd + HIDDEN, HIDDEN)] + [(HIDDEN, HIDDEN)] * 3
    if n_angles == 0:
        return trunk + [(HIDDEN, HIDDEN), (HIDDEN, LAST), (LAST, 3), (HIDDEN, 1)]
    return trunk + [(HIDDEN + dd, LAST), (LAST, 3), (HIDDEN + dd, 1)]


def scale_table(L, Ld, n_angles, w_xyz=None, w_dir=None):
    w_xyz = np.ones(L, np.float32) if w_xyz is None else np.asarray(w_xyz, np.float32)
    w_dir = np.ones(Ld, np.float32) if w_dir is None else np.asarray(w_dir, np.float32)
    assert w_xyz.shape == (L,) and w_dir.shape == (Ld,)
    parts = []
    for l, (rows, cols) in enumerate(layer_shapes(L, Ld, n_angles)):
        s = np.ones((rows, cols), np.float32)
        if l in (0, 4):
            for c in range(3):
                for k in range(L):
                    for h in range(2):
                        s[c * (1 + 2 * L) + 1 + 2 * k + h, :] = w_xyz[k]
        if n_angles != 0 and l in (8, 10):
            for c in range(n_angles + 1):
                for k in range(Ld):
                    for h in range(2):
                        s[HIDDEN + c * 2 * Ld + 2 * k + h, :] = w_dir[k]
        parts += [s.ravel(), np.ones(cols, np.float32)]
    return np.concatenate(parts)


def fold(blob, S):
    """fl32(blob * S): one float32 multiplication per element, as the re-pack performs it."""
    blob, S = np.asarray(blob, np.float32), np.asarray(S, np.float32)
    assert blob.shape == S.shape, (blob.shape, S.shape)
    return (blob * S).astype(np.float32)


def masks(L, Ld, n_angles, w_xyz, w_dir):
    """(xyz mask (3 + 6 L,), direction mask (2 Ld (n_angles + 1),) or None): the factor of every encoding feature."""
    mx = np.concatenate([np.concatenate([[1.0], np.repeat(np.asarray(w_xyz, np.float64), 2)]) for _ in range(3)])
    md = None if n_angles == 0 else np.concatenate([np.repeat(np.asarray(w_dir, np.float64), 2) for _ in range(n_angles + 1)])
    return mx, md


def cosine_window(alpha, n):
    """BARF: w_k = 0 for alpha < k, (1 - cos((alpha - k) pi)) / 2 for 0 <= alpha - k < 1, 1 above."""
    out = np.empty(n)
    for k in range(n):
        t = alpha - k
        out[k] = 0.0 if t < 0 else (1.0 if t >= 1 else (1.0 - np.cos(t * np.pi)) / 2.0)
    return out


def linear_window(alpha, n):
    return np.array([min(max(alpha - k, 0.0), 1.0) for k in range(n)])
