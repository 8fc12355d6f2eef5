"""Test-side restatement of the SH radiance volume (include/nerf_mi355.h: nerf_sh_radiance_lattice has the format, the basis and
the direction rule, nerf_sh_volume_sample the per-point rule): direction normalisation, the basis, the bake's projection sum,
the sampler and the march, in numpy float32 with the kernels' operations in the kernels' order, every operation rounded on its
own.  The cell and the lerps (trilinear), the march itself, its bar and the tests' media and rays are tests/volume_ref.py's;
nothing here touches the library.

A volume is (n, n, n, C) indexed [iz, iy, ix, channel]: channel 3 k + c the coefficient of basis function k for colour c,
channel 3 K the density, zeros after it; K = (L + 1)^2, C = 4 ceil((3 K + 1) / 4)."""
import numpy as np

from scene_box_ref import ray_box_interval  # noqa: F401 (re-exported)
from volume_ref import F, march as volume_march, march_bar, random_volume, rays_through_box, trilinear  # noqa: F401 (re-exported)

MAX_DEGREE, MAX_DIRS, CHUNK_POINTS = 3, 64, 1 << 20
C0 = F(0.28209479177387814)
C1 = F(0.4886025119029199)
C2 = (F(1.0925484305920792), F(0.31539156525252005), F(0.5462742152960396))
C3 = (F(0.5900435899266435), F(2.890611442640554), F(0.4570457994644658), F(0.3731763325901154), F(1.445305721320277))


def basis_count(degree):
    return (degree + 1) ** 2


def texel_floats(degree):
    return 4 * ((3 * basis_count(degree) + 1 + 3) // 4)


def vertices_per_pass(n_dirs):
    """The header's chunk rule: max(1, floor(2^20 / D)) vertices go through the network at a time."""
    return max(1, CHUNK_POINTS // n_dirs)


def unit(d):
    """(M, 3) -> d / |d| with s = (dx dx + dy dy) + dz dz, r = sqrt(s), one division per component; (0, 0, 1) where s is 0 or
    not finite."""
    d = np.asarray(d, F)[:, :3]
    with np.errstate(all="ignore"):
        s = (((d[:, 0] * d[:, 0]).astype(F) + (d[:, 1] * d[:, 1]).astype(F)).astype(F) + (d[:, 2] * d[:, 2]).astype(F)).astype(F)
        ok = (s != 0) & np.isfinite(s)
        r = np.sqrt(np.where(ok, s, F(1))).astype(F)
        u = (d / r[:, None]).astype(F)
    return np.where(ok[:, None], u, np.array([0, 0, 1], F)[None, :]).astype(F)


def basis(degree, u):
    """Y (M, K) float32 at unit vectors u (M, 3), in the header's operation order."""
    u = np.asarray(u, F)
    x, y, z = u[:, 0], u[:, 1], u[:, 2]

    def m(a, b):
        return (a * b).astype(F)

    def s(a, b):
        return (a - b).astype(F)
    out = [np.full(x.shape, C0, F)]
    if degree >= 1:
        out += [m(C1, y), m(C1, z), m(C1, x)]
    if degree >= 2:
        xx, yy, zz, xy, yz, xz = m(x, x), m(y, y), m(z, z), m(x, y), m(y, z), m(x, z)
        out += [m(C2[0], xy), m(C2[0], yz), m(C2[1], s(m(F(3), zz), F(1))), m(C2[0], xz), m(C2[2], s(xx, yy))]
    if degree >= 3:
        zz5 = m(F(5), zz)
        out += [m(C3[0], m(y, s(m(F(3), xx), yy))), m(C3[1], m(xy, z)), m(C3[2], m(y, s(zz5, F(1)))),
                m(C3[3], m(z, s(zz5, F(3)))), m(C3[2], m(x, s(zz5, F(1)))), m(C3[4], m(z, s(xx, yy))),
                m(C3[0], m(x, s(xx, m(F(3), yy))))]
    return np.stack(out, axis=1)


def project(proj, colours):
    """The bake's sum: proj (K, D), colours (V, D, 3) -> coefficients (V, K, 3): proj[k][0] colour_0, then + proj[k][j] colour_j
    for j = 1 .. D - 1 in order, each multiply and each add rounded on its own."""
    proj, colours = np.asarray(proj, F), np.asarray(colours, F)
    acc = (proj[None, :, 0, None] * colours[:, None, 0, :]).astype(F)
    for j in range(1, proj.shape[1]):
        acc = (acc + (proj[None, :, j, None] * colours[:, None, j, :]).astype(F)).astype(F)
    return acc


def texels(coef, sigma):
    """coef (..., K, 3), sigma (...) -> texels (..., C): the format's channel order, zero padding."""
    coef, sigma = np.asarray(coef, F), np.asarray(sigma, F)
    k = coef.shape[-2]
    degree = int(round(np.sqrt(k))) - 1
    assert basis_count(degree) == k
    out = np.zeros(sigma.shape + (texel_floats(degree),), F)
    out[..., :3 * k] = coef.reshape(sigma.shape + (3 * k,))
    out[..., 3 * k] = sigma
    return out


def degree_of(volume):
    c = volume.shape[-1]
    degree = {texel_floats(d): d for d in range(MAX_DEGREE + 1)}[c]
    return degree


def embed(volume, degree):
    """The same volume stored at a higher degree: zero coefficients above its own."""
    low = degree_of(volume)
    k = basis_count(low)
    coef = np.zeros(volume.shape[:-1] + (basis_count(degree), 3), F)
    coef[..., :k, :] = volume[..., :3 * k].reshape(volume.shape[:-1] + (k, 3))
    return texels(coef, volume[..., 3 * k])


def random_sh_volume(n, degree, seed, sigma_scale=3.0, coef_scale=1.0):
    """Coefficients uniform in [-1, 1) times coef_scale -- the clamp at 0 acts on some samples, from coef_scale 4 on the clamp
    at 1 too -- and volume_ref.random_volume's density."""
    rng = np.random.default_rng(seed)
    coef = ((rng.random((n, n, n, basis_count(degree), 3), dtype=F) * F(2) - F(1)) * F(coef_scale)).astype(F)
    return texels(coef, random_volume(n, seed, sigma_scale)[..., 3])


def orbit(c2w, centre, degrees):
    """The camera c2w (4, 4) carried ``degrees`` of azimuth around ``centre`` about its own up axis (column 1), still looking
    at what it looked at -> (4, 4) float32."""
    c = np.asarray(c2w, np.float64).reshape(4, 4)
    k = c[:3, 1] / np.linalg.norm(c[:3, 1])
    kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    t = np.radians(degrees)
    rot = np.eye(3) + np.sin(t) * kx + (1 - np.cos(t)) * (kx @ kx)
    out = c.copy()
    out[:3, :3] = rot @ c[:3, :3]
    out[:3, 3] = np.asarray(centre, np.float64) + rot @ (c[:3, 3] - np.asarray(centre, np.float64))
    return out.astype(F)


def clamp01(x):
    return np.where(x < 0, F(0), np.where(x > 1, F(1), x)).astype(F)      # a NaN fails both comparisons and stays


def sample_unclamped(volume, lo, hi, points, y):
    """(M, 4) before the clamp, with the basis values y (M, K) given."""
    k = basis_count(degree_of(np.asarray(volume)))

    def vertex(t):
        coef = t[:, :3 * k].reshape(-1, k, 3)
        with np.errstate(all="ignore"):
            acc = (y[:, 0, None] * coef[:, 0]).astype(F)
            for b in range(1, k):
                acc = (acc + (y[:, b, None] * coef[:, b]).astype(F)).astype(F)
        return np.concatenate([acc, t[:, 3 * k, None]], axis=1)
    return trilinear(volume, lo, hi, points, vertex)


def sample(volume, lo, hi, points, dirs, y=None):
    """(M, 4): the colour towards dirs / |dirs| clamped to [0, 1], and the density."""
    if y is None:
        y = basis(degree_of(np.asarray(volume)), unit(dirs))
    out = sample_unclamped(volume, lo, hi, points, y)
    out[:, :3] = clamp01(out[:, :3])
    return out


def march(volume, lo, hi, near, far, rays_orig, rays_dirs, n_steps, t_min=0.0, exp=None, count_clamped=None):
    """volume_ref.march with this module's sample; u and Y once per ray.  ``count_clamped``: a list that receives the number of
    live samples whose colour the clamp changed."""
    y = basis(degree_of(np.asarray(volume)), unit(np.asarray(rays_dirs, F)))
    clamped = [0]

    def value(p, alive):
        raw = sample_unclamped(volume, lo, hi, p, y)
        v = raw.copy()
        v[:, :3] = clamp01(raw[:, :3])
        clamped[0] += int((v[alive, :3] != raw[alive, :3]).any(axis=1).sum())
        return v
    out = volume_march(volume, lo, hi, near, far, rays_orig, rays_dirs, n_steps, t_min, exp, value)
    if count_clamped is not None:
        count_clamped.append(clamped[0])
    return out
