"""The SH radiance volume without a GPU: the projection tables the package hands out (sh_quadrature, sh_least_squares), the
float32 restatement of tests/sh_volume_ref.py (what tests/test_gpu_sh_volume.py holds the kernels to) against the properties
the format is meant to have, and the interface (header, binding, package)."""
import os
import re

import numpy as np
import pytest

import sh_volume_ref as SH
import support as S
from volume_ref import HI, LO

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"nerf_sh_radiance_lattice": 9, "nerf_sh_volume_sample": 11, "nerf_sh_volume_march": 15, "nerf_sh_volume_render_image": 18}
NEAR, FAR = 2.0, 6.0


def random_unit(n, seed):
    g = np.random.default_rng(seed).normal(size=(n, 3))
    return g / np.linalg.norm(g, axis=1, keepdims=True)


# ---- the tables -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_default_table_projects_the_basis_onto_itself(degree):
    import nerf_and_dietnerf_amd as N
    dirs, proj = N.sh_quadrature(degree)
    k, d = (degree + 1) ** 2, (degree + 1) * (2 * degree + 1)
    assert d == (1, 6, 15, 28)[degree] and N.sh_basis_count(degree) == k
    assert dirs.shape == (d, 3) and dirs.dtype == F and proj.shape == (k, d) and proj.dtype == F
    np.testing.assert_allclose(np.linalg.norm(dirs.astype(np.float64), axis=1), 1.0, atol=1e-6)
    # node-major: the 2 L + 1 directions of a node share z, and the nodes' z ascend
    z = dirs[:, 2].reshape(degree + 1, 2 * degree + 1)
    assert (np.abs(z - z[:, :1]) <= 1e-7).all() and (np.diff(z[:, 0]) > 0).all()
    gram = proj.astype(np.float64) @ N.sh_basis(degree, dirs.astype(np.float64))
    err = float(np.abs(gram - np.eye(k)).max())
    print(f"[default table, degree {degree}] max |proj Y - I| = {err:.2e}, bar 1e-6")
    assert err <= 1e-6
    # the restatement's float32 basis is the package's float64 one
    u = random_unit(500, degree)
    assert np.abs(SH.basis(degree, u.astype(F)) - N.sh_basis(degree, u.astype(F))).max() <= 4 * 2.0 ** -23
    assert N.sh_texel_floats(degree) == SH.texel_floats(degree) == (4, 16, 28, 52)[degree]


@pytest.mark.parametrize("degree", [1, 2, 3])
def test_least_squares_table_on_one_hemisphere(degree):
    import nerf_and_dietnerf_amd as N
    dirs = random_unit(40, 10 + degree)
    dirs[:, 2] = np.abs(dirs[:, 2])                       # what cameras above the object see
    proj = N.sh_least_squares(degree, dirs * 1.7)         # any length: the fit is over dirs / |dirs|
    k = (degree + 1) ** 2
    assert proj.shape == (k, 40) and proj.dtype == F
    coef = np.random.default_rng(degree).uniform(-1, 1, (k, 3))
    colours = N.sh_basis(degree, dirs) @ coef             # a degree-<=L colour function at those directions
    fitted = N.sh_basis(degree, dirs) @ (proj.astype(np.float64) @ colours)
    err = float(np.abs(fitted - colours).max())
    print(f"[least-squares table, degree {degree}] max error at the 40 directions {err:.2e}, bar 1e-5")
    assert err <= 1e-5
    with pytest.raises(ValueError, match="at least"):
        N.sh_least_squares(degree, dirs[:k - 1])
    with pytest.raises(ValueError, match="rank-deficient"):
        N.sh_least_squares(degree, np.tile(dirs[:2], (20, 1)))
    with pytest.raises(ValueError, match="zero vector"):
        N.sh_least_squares(degree, np.concatenate([dirs, np.zeros((1, 3))]))
    with pytest.raises(ValueError, match="SH degree must be in 0..3"):
        N.sh_least_squares(4, dirs)


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_sampling_reproduces_a_known_function_and_clamps(degree):
    import nerf_and_dietnerf_amd as N
    n, k = 5, (degree + 1) ** 2
    rng = np.random.default_rng(20 + degree)
    coef = rng.uniform(-0.5, 0.5, (k, 3))
    coef[0] = (0.5 / 0.28209479177387814, 6.0, -3.0)      # red around 0.5; green around 1.7 and blue around -0.85: clamped
    vol = SH.texels(np.broadcast_to(coef.astype(F), (n, n, n, k, 3)), np.full((n, n, n), 0.75, F))
    u = random_unit(1000, 30 + degree)
    p = rng.uniform(np.array(LO), np.array(HI), (1000, 3)).astype(F)
    got = SH.sample(vol, LO, HI, p, (u * rng.uniform(0.3, 3.0, (1000, 1))).astype(F))
    want = N.sh_basis(degree, u) @ coef.astype(F).astype(np.float64)
    magnitude = float(np.abs(N.sh_basis(degree, u)[:, :, None] * coef[None]).sum(axis=1).max())
    bar = (k + 8) * float(np.spacing(F(magnitude)))       # k products and sums, the direction's and the lerps' roundings
    inside = (want > 0) & (want < 1)
    err = float(np.abs(got[:, :3] - want)[inside].max())
    print(f"[known function, degree {degree}] max error {err:.2e}, bar {bar:.2e}; {int((~inside).sum())} of {inside.size} clamped")
    assert got.dtype == F and err <= bar
    assert (S.bits(got[:, 3]) == S.bits(F(0.75))).all()
    below, above = want < -bar, want > 1 + bar
    assert below.sum() > 100 and above.sum() > 100 and inside.sum() > 500
    assert (S.bits(got[:, :3][below]) == 0).all() and (S.bits(got[:, :3][above]) == S.bits(F(1))).all()
    vol[..., 0] = np.nan
    assert np.isnan(SH.sample(vol, LO, HI, p[:4], u[:4].astype(F))[:, 0]).all()      # a NaN stays NaN through the clamp


def test_direction_normalisation():
    odd = np.array([[0, 0, 0], [-0.0, 0.0, -0.0], [np.inf, 0, 0], [0, -np.inf, 1], [np.nan, 1, 1], [3e38, 1, 1], [1, 3e38, -3e38]], F)
    np.testing.assert_array_equal(SH.unit(odd), np.tile(np.array([0, 0, 1], F), (len(odd), 1)))
    d = (random_unit(500, 40) * np.random.default_rng(41).uniform(1e-3, 1e3, (500, 1))).astype(F)
    u = SH.unit(d)
    assert u.dtype == F
    want = d.astype(np.float64) / np.linalg.norm(d.astype(np.float64), axis=1, keepdims=True)
    assert np.abs(u - want).max() <= 3 * 2.0 ** -24       # the sum, the root and the division: half an ulp each, of values <= 1
    tiny = np.array([[1e-30, 0, 0], [0, -2e-25, 0]], F)    # |d|^2 underflows to 0: the zero rule
    np.testing.assert_array_equal(SH.unit(tiny), np.tile(np.array([0, 0, 1], F), (2, 1)))


@pytest.mark.parametrize("low,high", [(0, 1), (1, 3), (2, 3), (0, 3)])
def test_zero_padding_embeds_a_lower_degree(low, high):
    n = 5
    vol = SH.random_sh_volume(n, low, 50 + low)
    big = SH.embed(vol, high)
    assert big.shape == (n, n, n, SH.texel_floats(high)) and SH.degree_of(big) == high
    rng = np.random.default_rng(60)
    p = rng.uniform(np.array(LO) - 0.2, np.array(HI) + 0.2, (300, 3)).astype(F)
    d = rng.normal(size=(300, 3)).astype(F)
    S.assert_same_bits(SH.sample(big, LO, HI, p, d), SH.sample(vol, LO, HI, p, d))
    o4, d4 = SH.rays_through_box(48, 61)
    for a, b in zip(SH.march(big, LO, HI, NEAR, FAR, o4, d4, 7), SH.march(vol, LO, HI, NEAR, FAR, o4, d4, 7)):
        S.assert_same_bits(a, b)


def test_degree_zero_is_the_plain_volume_times_y0():
    """A degree-0 volume whose coefficient is colour / Y_0 marches to the plain volume's result up to that one rounding."""
    import volume_ref as V
    plain = V.random_volume(5, 70)
    vol = plain.copy()
    vol[..., :3] = (plain[..., :3] / SH.C0).astype(F)
    o4, d4 = SH.rays_through_box(48, 71)
    got, want = SH.march(vol, LO, HI, NEAR, FAR, o4, d4, 7), V.march(plain, LO, HI, NEAR, FAR, o4, d4, 7)
    assert np.abs(got[0] - want[0]).max() <= 4 * 2.0 ** -23
    S.assert_same_bits(got[2], want[2])                   # the density path is the same code


def test_projection_sum_recovers_coefficients():
    import nerf_and_dietnerf_amd as N
    for degree in range(4):
        dirs, proj = N.sh_quadrature(degree)
        k = (degree + 1) ** 2
        coef = np.random.default_rng(80 + degree).uniform(-1, 1, (7, k, 3))
        colours = np.einsum("dk,vkc->vdc", N.sh_basis(degree, dirs.astype(np.float64)), coef).astype(F)
        got = SH.project(proj, colours)
        assert got.shape == (7, k, 3) and got.dtype == F
        assert np.abs(got - coef).max() <= 1e-5


def test_chunk_rule():
    assert SH.vertices_per_pass(28) == 37449 and 33 ** 3 <= 37449 < 34 ** 3
    assert SH.vertices_per_pass(1) == 1 << 20 and SH.vertices_per_pass(64) == 16384


# ---- the interface ------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_bound_wrapped_and_exported():
    import nerf_and_dietnerf_amd as N
    text = open(os.path.join(ROOT, "include", "nerf_mi355.h")).read()
    declared = set(re.findall(r"\b(nerf_[a-z_]+)\s*\(", text))
    bound = {name: args for name, _, args in N._lib.SYMBOLS}
    lib = N._lib.load()
    for name, nargs in NEW.items():
        assert name in declared, name
        assert name in bound and len(bound[name]) == nargs, name
        assert getattr(lib, name) is not None
    assert re.search(r"#define\s+NERF_ABI_VERSION\s+6\b", text) and N._lib.NERF_ABI_VERSION == 6 and lib.nerf_abi_version() == 6
    for method in ("sh_radiance_lattice", "sample_sh_volume", "march_sh_volume", "render_sh_volume_image"):
        assert callable(getattr(N.Context, method))
    for helper in ("sh_basis", "sh_quadrature", "sh_least_squares"):
        assert callable(getattr(N, helper)) and helper in N.__all__
    import inspect
    params = inspect.signature(N.NeRF.bake_preview).parameters
    assert [params[k].default for k in ("sh_degree", "sh_dirs", "sh_proj")] == [None, None, None]
    assert N.DietNeRF.bake_preview is N.NeRF.bake_preview
    # the rules the header owes its reader
    doc = text[text.index("view-dependent colour in the radiance volume"):text.index("int nerf_sh_volume_render_image")]
    doc = re.sub(r"\s*\n \*\s*", " ", doc)
    for phrase in ("Channel 3 k + c holds the coefficient of basis function k for colour channel c", "a NaN stays NaN",
                   "u = (0, 0, 1)", "max(1, floor(2^20 / D)) vertices", "the network sees that length",
                   "includes directions no camera saw", "0.31539156525252005 ((3 zz) - 1)"):
        assert phrase in doc, phrase
