"""Spherical harmonics for the SH radiance volume (include/nerf_mi355.h: nerf_sh_radiance_lattice has the format): the real
orthonormal basis up to degree 3 in float64, the default projection table (a quadrature that is exact for the products of two
basis functions) and a least-squares table over a caller's own directions.  Host arithmetic only; the device evaluates the
same basis in float32."""
import numpy as np

SH_MAX_DEGREE = 3
SH_MAX_DIRS = 64


def sh_basis_count(degree: int) -> int:
    """K = (degree + 1)^2."""
    return (check_sh_degree(degree) + 1) ** 2


def sh_texel_floats(degree: int) -> int:
    """C(L) = 4 ceil((3 K + 1) / 4): 4 / 16 / 28 / 52 float32 per vertex."""
    return 4 * ((3 * sh_basis_count(degree) + 1 + 3) // 4)


def sh_degree_of(channels: int) -> int:
    """The degree whose texel has ``channels`` floats; ValueError if none has."""
    for degree in range(SH_MAX_DEGREE + 1):
        if sh_texel_floats(degree) == channels:
            return degree
    sizes = ", ".join(str(sh_texel_floats(d)) for d in range(SH_MAX_DEGREE + 1))
    raise ValueError(f"an SH volume has {sizes} channels for degree 0..{SH_MAX_DEGREE} (got {channels})")


def check_sh_degree(degree) -> int:
    if int(degree) != degree or not 0 <= degree <= SH_MAX_DEGREE:
        raise ValueError(f"SH degree must be in 0..{SH_MAX_DEGREE} (got {degree!r})")
    return int(degree)


def sh_basis(degree: int, dirs) -> np.ndarray:
    """The K = (degree + 1)^2 basis functions at ``dirs`` (..., 3) -> (..., K) float64.  ``dirs`` are used as given: pass unit
    vectors (the functions are polynomials in x, y, z, orthonormal on the unit sphere)."""
    k = sh_basis_count(degree)
    d = np.asarray(dirs, np.float64)
    if d.shape[-1:] != (3,):
        raise ValueError(f"dirs must be a (..., 3) array, got {d.shape}")
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    xx, yy, zz = x * x, y * y, z * z
    rows = [0.28209479177387814 * np.ones_like(x),
            0.4886025119029199 * y, 0.4886025119029199 * z, 0.4886025119029199 * x,
            1.0925484305920792 * x * y, 1.0925484305920792 * y * z, 0.31539156525252005 * (3.0 * zz - 1.0),
            1.0925484305920792 * x * z, 0.5462742152960396 * (xx - yy),
            0.5900435899266435 * y * (3.0 * xx - yy), 2.890611442640554 * x * y * z, 0.4570457994644658 * y * (5.0 * zz - 1.0),
            0.3731763325901154 * z * (5.0 * zz - 3.0), 0.4570457994644658 * x * (5.0 * zz - 1.0),
            1.445305721320277 * z * (xx - yy), 0.5900435899266435 * x * (xx - 3.0 * yy)]
    return np.stack(rows[:k], axis=-1)


def sh_quadrature(degree: int):
    """The default table of Context.sh_radiance_lattice -> (dirs (D, 3) float32, proj (K, D) float32): the degree + 1
    Gauss-Legendre nodes in cos(theta) times 2 degree + 1 equally spaced azimuths (m + 1/2) 2 pi / (2 degree + 1), node-major,
    D = 1 / 6 / 15 / 28; proj[k][j] = q_j Y_k(dirs_j) in float64, rounded once.  Exact for the products of two basis functions,
    so projecting a function of degree <= ``degree`` returns its coefficients."""
    degree = check_sh_degree(degree)
    nodes, weights = np.polynomial.legendre.leggauss(degree + 1)
    m = 2 * degree + 1
    phi = (np.arange(m) + 0.5) * (2.0 * np.pi / m)
    ct = np.repeat(nodes, m)
    st = np.sqrt(1.0 - ct * ct)
    dirs = np.stack([st * np.tile(np.cos(phi), degree + 1), st * np.tile(np.sin(phi), degree + 1), ct], axis=1)
    q = np.repeat(weights, m) * (2.0 * np.pi / m)
    proj = (sh_basis(degree, dirs) * q[:, None]).T
    return dirs.astype(np.float32), np.ascontiguousarray(proj, np.float32)


def sh_least_squares(degree: int, dirs) -> np.ndarray:
    """proj (K, D) float32 = pinv(Y(dirs / |dirs|)) for a caller's own directions (D, 3): the coefficients that fit the D
    colours best.  The typical set is the directions from which the training cameras saw the object -- towards directions
    nobody photographed the network's colour is noise, and a full-sphere table spends coefficients on it.  Refuses D < K and a
    set on which the basis functions are not independent."""
    k = sh_basis_count(degree)
    d = np.asarray(dirs, np.float64)
    if d.ndim != 2 or d.shape[1] != 3:
        raise ValueError(f"dirs must be a (D, 3) array, got {d.shape}")
    if not np.isfinite(d).all():
        raise ValueError("sh_least_squares: dirs has a non-finite entry")
    norm = np.linalg.norm(d, axis=1)
    if (norm == 0).any():
        raise ValueError(f"sh_least_squares: dirs[{int(np.argmax(norm == 0))}] is the zero vector")
    if d.shape[0] < k:
        raise ValueError(f"sh_least_squares: degree {degree} needs at least {k} directions (got {d.shape[0]})")
    basis = sh_basis(degree, d / norm[:, None])
    s = np.linalg.svd(basis, compute_uv=False)
    if s[-1] <= 1e-6 * s[0]:
        raise ValueError(f"sh_least_squares: the directions are rank-deficient for degree {degree} (singular values "
                         f"{s[0]:.3g} .. {s[-1]:.3g})")
    return np.ascontiguousarray(np.linalg.pinv(basis), np.float32)
