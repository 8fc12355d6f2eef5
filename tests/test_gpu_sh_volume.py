"""The SH radiance volume on the device: the sampler against the numpy restatement of tests/sh_volume_ref.py bit for bit, the
bake against the public point queries (mesh_colors, density_lattice) and the restatement's projection sum bit for bit -- also
across the chunk seam --, the march against the restatement up to expf, the invariances (zero padding, batching, host /
device arrays, the image call), the refusals, and NeRF.bake_preview(sh_degree=...) / render_preview on the shipped checkpoint."""
import numpy as np
import pytest

from isosurface_ref import lattice_points
from occupancy_ref import GOLDEN_BOX
import sh_volume_ref as SH
import support as S
from volume_ref import FAR, HI, LO, NEAR, march_bar, march_rays, rays_through_box, same_f32, sample_points

pytestmark = pytest.mark.gpu

F = np.float32
DEGREES = (0, 1, 2, 3)


@pytest.fixture(scope="module")
def ctx():
    """A context for the calls that need no network."""
    import nerf_and_dietnerf_amd as N
    c = N.Context(precision="fp32", near=NEAR, far=FAR)
    yield c
    c.close()


# ---- 1. sampling equals the restatement bit for bit -----------------------------------------------------------------------------
def sample_dirs(m=257, seed=1):
    """Unit, un-normalised (1e-3 .. 1e3), axis-aligned, zero, non-finite and overflowing directions -> (m, 3), shuffled so
    that the odd ones do not meet the odd points."""
    rng = np.random.default_rng(seed)
    odd = np.array([[0, 0, 0], [-0.0, 0, 0], [np.nan, 1, 0], [0, np.inf, 0], [1, 1, -np.inf], [3e38, 3e38, 0], [1, 0, 0],
                    [0, -1, 0], [0, 0, -2], [1e-30, 0, 0]], F)
    g = rng.normal(size=(m - len(odd), 3))
    g = g / np.linalg.norm(g, axis=1, keepdims=True)
    g[::3] *= rng.uniform(1e-3, 1e3, (len(g[::3]), 1))
    return np.concatenate([odd, g.astype(F)])[rng.permutation(m)]


@pytest.mark.parametrize("n", [2, 3, 9])
@pytest.mark.parametrize("degree", DEGREES)
def test_sampling_equals_the_restatement(ctx, degree, n):
    import torch
    v = SH.random_sh_volume(n, degree, 10 * degree + n, coef_scale=4.0)       # Y_0 coef reaches 1.13: the clamp acts both ways
    p, has_nan = sample_points(n)
    d = sample_dirs()
    assert p.shape == d.shape == (257, 3) and has_nan.sum() == 4
    unit = SH.unit(d)
    assert ((unit == np.array([0, 0, 1], F)).all(axis=1)).sum() >= 7          # the zero, non-finite and overflowing directions
    got = ctx.sample_sh_volume(v, LO, HI, p, d)
    want = SH.sample(v, LO, HI, p, d)
    assert got.shape == (257, 4) and got.dtype == F
    np.testing.assert_array_equal(np.isnan(got).any(axis=1), has_nan)        # NaN out only for NaN in (a point's: never a direction's)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_array_equal(S.bits(got)[~has_nan], S.bits(want)[~has_nan])
    rgb = got[~has_nan, :3]
    assert rgb.min() >= 0 and rgb.max() <= 1 and (rgb == 0).any() and ((rgb == 1).any() or n < 9)      # the clamp acts, both ways
    dev = ctx.sample_sh_volume(torch.as_tensor(v).cuda(), LO, HI, torch.as_tensor(p).cuda(), torch.as_tensor(d).cuda())
    assert dev.is_cuda
    np.testing.assert_array_equal(S.bits(dev.cpu().numpy())[~has_nan], S.bits(got)[~has_nan])


# ---- 2. the bake -----------------------------------------------------------------------------------------------------------------
def check_bake(c, which, n, degree, dirs, proj, vol, vertices=None):
    """vol (n, n, n, C) against the projection sum over mesh_colors along every direction of the table, density_lattice and
    the zero padding, at all vertices or at those listed."""
    k = SH.basis_count(degree)
    assert vol.shape == (n, n, n, SH.texel_floats(degree)) and vol.dtype == F
    pts = lattice_points(c.scene_box[0], c.scene_box[1], n)
    flat = vol.reshape(len(pts), -1)
    sigma = c.density_lattice(which, n, view_dir=dirs[0]).reshape(-1)
    if vertices is not None:
        pts, flat, sigma = pts[vertices], flat[vertices], sigma[vertices]
    colours = np.stack([c.mesh_colors(which, pts, np.tile(-dirs[j], (len(pts), 1))) for j in range(len(dirs))], axis=1)
    same_f32(flat[:, :3 * k].reshape(-1, k, 3), SH.project(proj, colours), "coefficients")
    same_f32(flat[:, 3 * k], np.maximum(sigma, F(0)), "sigma")
    assert (S.bits(flat[:, 3 * k + 1:]) == 0).all()
    assert flat.shape[1] - (3 * k + 1) == (0, 3, 0, 3)[degree]
    return flat


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_bake_equals_the_projection_of_the_point_queries(precision):
    import nerf_and_dietnerf_amd as N
    c = S.glorot_context(precision)
    c.set_scene_box(LO, HI)
    n = 5
    for degree in (1, 2, 3):
        dirs, proj = N.sh_quadrature(degree)
        flat = check_bake(c, 1, n, degree, dirs, proj, c.sh_radiance_lattice(1, n, degree))
        assert np.unique(flat[:, 0]).size > n and np.abs(flat[:, 3:3 * SH.basis_count(degree)]).max() > 1e-4      # a field, view-dependent
    # a caller's table: un-normalised directions of one hemisphere, least squares; the coarse network (its sigma is lifted)
    rng = np.random.default_rng(5)
    own = rng.normal(size=(12, 3))
    own[:, 2] = np.abs(own[:, 2])
    own = own.astype(F)
    proj = N.sh_least_squares(2, own)
    vol = c.sh_radiance_lattice(0, n, 2, dirs=own, proj=proj)
    flat = check_bake(c, 0, n, 2, own, proj, vol)
    assert (flat[:, 27] > 0).any()
    dev = c.sh_radiance_lattice(0, n, 2, dirs=own, proj=proj, device_out=True)
    assert dev.is_cuda and tuple(dev.shape) == (n, n, n, 28)
    same_f32(dev.cpu().numpy(), vol)
    c.close()


@pytest.mark.parametrize("n_angles", [1, 0])
def test_bake_other_direction_inputs(n_angles):
    import nerf_and_dietnerf_amd as N
    c = S.glorot_context("f16x3", n_angles=n_angles)
    c.set_scene_box(LO, HI)
    dirs, proj = N.sh_quadrature(2)
    vol = c.sh_radiance_lattice(0, 5, 2)
    check_bake(c, 0, 5, 2, dirs, proj, vol)
    if n_angles == 0:                                                        # the directions are ignored: any table's directions do
        same_f32(c.sh_radiance_lattice(0, 5, 2, dirs=dirs[::-1].copy() * F(3), proj=proj), vol)
    c.close()


def test_bake_wide_encoding_network():
    import nerf_and_dietnerf_amd as N
    kw = dict(n_pos_enc_xyz=10, n_pos_enc_dir=4, n_angles=2)
    c = N.Context(precision="f16x3", **kw)
    blob = N.glorot_blob(1, **kw)
    blob[-1] = 0.5
    c.load_weights(0, blob)
    c.set_scene_box(LO, HI)
    dirs, proj = N.sh_quadrature(1)
    check_bake(c, 0, 5, 1, dirs, proj, c.sh_radiance_lattice(0, 5, 1))
    c.close()


# ---- 3. the chunk seam -----------------------------------------------------------------------------------------------------------
def test_bake_across_the_chunk_seam():
    import nerf_and_dietnerf_amd as N
    dirs, proj = N.sh_quadrature(3)
    per_pass = SH.vertices_per_pass(len(dirs))
    assert len(dirs) == 28 and 34 ** 3 > per_pass >= 33 ** 3
    c = S.glorot_context("f16x3")
    c.set_scene_box(LO, HI)
    vol = c.sh_radiance_lattice(0, 34, 3, device_out=True).cpu().numpy()
    picked = np.unique(np.concatenate([np.arange(0, 34 ** 3, 97), np.arange(per_pass - 8, per_pass + 8), [34 ** 3 - 1]]))
    assert (picked < per_pass).sum() > 100 and (picked >= per_pass).sum() > 10
    check_bake(c, 0, 34, 3, dirs, proj, vol, picked)
    c.close()


# ---- 4. the march against the restatement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,n_rays", [(5, 37), (9, 257)])
@pytest.mark.parametrize("degree", DEGREES)
def test_march_against_the_restatement(ctx, degree, n, n_rays):
    v = SH.random_sh_volume(n, degree, 10 + n)            # the density of tests/test_gpu_volume.py's march: no hit stays empty
    o, d = march_rays(n_rays, n)
    a, b, hit, _ = SH.ray_box_interval(o, d, LO, HI, NEAR, FAR)
    finite = np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1)
    hit &= finite
    assert (~finite).sum() == 1 and (~hit).sum() >= 5
    assert (hit & (a == F(NEAR))).any() and (hit & (b == F(FAR))).any() and (hit & (a > F(NEAR)) & (b < F(FAR))).any()
    assert (hit & (d[:, 0] == 0)).any() and (~hit & (d[:, 0] == 0)).any()
    for n_steps in (1, 2, 7, 48):
        rgb, depth, opacity = ctx.march_sh_volume(v, LO, HI, o, d, n_steps)
        clamped = []
        w_rgb, w_depth, w_opacity = SH.march(v, LO, HI, NEAR, FAR, o, d, n_steps, count_clamped=clamped)
        assert clamped[0] > 0                                                 # coefficients in +-1: the clamp acts on some samples
        assert rgb.shape == (n_rays, 3) and depth.shape == (n_rays,) and opacity.shape == (n_rays,)
        bar = march_bar(n_steps)
        errs = (float(np.abs(rgb - w_rgb).max()), float(np.abs(opacity - w_opacity).max()), float(np.abs(depth - w_depth).max()))
        print(f"[SH march degree {degree}, n={n}, {n_rays} rays, {n_steps} steps] rgb {errs[0]:.2e} opacity {errs[1]:.2e} "
              f"(bar {bar:.2e}) depth {errs[2]:.2e} (bar {bar * FAR:.2e}); {clamped[0]} samples clamped")
        assert errs[0] <= bar and errs[1] <= bar and errs[2] <= bar * FAR
        for out in (rgb, depth, opacity):                                     # misses and the NaN ray: exact zeros
            assert (S.bits(out)[~hit] == 0).all()
        assert (opacity[hit] > 0).all() and (opacity <= 1).all()


# ---- 5. invariances, bit for bit ----------------------------------------------------------------------------------------------------
def test_zero_padding_embeds_degree_one_in_three(ctx):
    v1 = SH.random_sh_volume(9, 1, 200)
    v3 = SH.embed(v1, 3)
    p, has_nan = sample_points(9)
    d = sample_dirs()
    got1, got3 = ctx.sample_sh_volume(v1, LO, HI, p, d), ctx.sample_sh_volume(v3, LO, HI, p, d)
    np.testing.assert_array_equal(S.bits(got3)[~has_nan], S.bits(got1)[~has_nan])
    o, r = march_rays(257, 201)
    for x, y in zip(ctx.march_sh_volume(v3, LO, HI, o, r, 7), ctx.march_sh_volume(v1, LO, HI, o, r, 7)):
        same_f32(x, y)


@pytest.mark.parametrize("degree", [0, 2, 3])
def test_march_of_halves_and_of_device_arrays(ctx, degree):
    import torch
    v = SH.random_sh_volume(9, degree, 210 + degree)
    o, d = march_rays(257, 211)
    whole = ctx.march_sh_volume(v, LO, HI, o, d, 7)
    first, second = ctx.march_sh_volume(v, LO, HI, o[:125], d[:125], 7), ctx.march_sh_volume(v, LO, HI, o[125:], d[125:], 7)
    dev = ctx.march_sh_volume(torch.as_tensor(v).cuda(), LO, HI, torch.as_tensor(o).cuda(), torch.as_tensor(d).cuda(), 7)
    for k in range(3):
        same_f32(np.concatenate([first[k], second[k]]), whole[k])
        assert dev[k].is_cuda
        same_f32(dev[k].cpu().numpy(), whole[k])


def test_t_min_changes_rgb_and_opacity_by_at_most_t_min(ctx):
    tau = 1e-2
    v = SH.random_sh_volume(9, 2, 220, sigma_scale=40.0)
    o, d = rays_through_box(257, 221)
    _, b, hit, _ = SH.ray_box_interval(o, d, LO, HI, NEAR, FAR)
    full, cut = ctx.march_sh_volume(v, LO, HI, o, d, 48), ctx.march_sh_volume(v, LO, HI, o, d, 48, t_min=tau)
    assert hit.all() and (S.bits(cut[2]) != S.bits(full[2])).sum() > 16       # the cut acts on this medium
    assert np.abs(cut[0] - full[0]).max() <= tau and np.abs(cut[2] - full[2]).max() <= tau
    assert (np.abs(cut[1] - full[1]) <= tau * b).all()


@pytest.mark.parametrize("ndc", [False, True])
def test_image_call_equals_rays_plus_march(oracle, ndc):
    import nerf_and_dietnerf_amd as N
    import torch
    h, w, fov, n_steps = 13, 11, 0.6911112, 7
    v = SH.random_sh_volume(9, 2, 230)
    if ndc:
        c = N.Context(precision="fp32", near=0.0, far=1.0)
        c.set_ray_space("ndc", 1.0)
        c2w = oracle.get_sphere_matrix(0.5, 0.0, 0.0, 0.0).astype(F)           # looking down -z
        c2w[0, 3], c2w[1, 3] = 0.03, -0.02
        lo, hi = (-0.9, -1.0, -1.0), (1.0, 0.8, 0.7)
    else:
        c = N.Context(precision="fp32", near=NEAR, far=FAR)
        c2w = oracle.get_sphere_matrix(4.0, -30.0, 45.0, 10.0).astype(F)
        lo, hi = LO, HI
    d = c.get_rays_directions(h, w, fov, c2w).reshape(-1, 4)
    o = np.tile(c2w[:, 3], (h * w, 1)).astype(F)
    if ndc:
        o, d = c.rays_to_ndc(o, d, fov, 1.0)
    want = c.march_sh_volume(v, lo, hi, o, d, n_steps)
    assert (want[2] > 0).sum() > h * w // 4                                   # the camera sees the volume
    got = c.render_sh_volume_image(v, lo, hi, c2w, fov, h, w, n_steps)
    assert got[0].shape == (h, w, 3) and got[1].shape == (h, w) and got[2].shape == (h, w)
    for k in range(3):
        same_f32(got[k].reshape(want[k].shape), want[k])
    for begin, count in ((0, 5), (5, 40), (45, h * w - 45)):                  # slabs that split rows of 11
        part = c.render_sh_volume_image(v, lo, hi, c2w, fov, h, w, n_steps, ray_begin=begin, ray_count=count)
        for k in range(3):
            same_f32(part[k], want[k][begin:begin + count])
    dev = c.render_sh_volume_image(torch.as_tensor(v).cuda(), lo, hi, c2w, fov, h, w, n_steps)
    for k in range(3):
        same_f32(dev[k].cpu().numpy(), got[k])
    c.close()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals(oracle):
    import nerf_and_dietnerf_amd as N
    last = N._lib.last_error
    c = N.Context(precision="fp32", near=NEAR, far=FAR)
    dirs, proj = N.sh_quadrature(1)
    out = np.zeros(3 ** 3 * 52, F)

    def bake(which=0, n=3, degree=1, dirs=dirs, proj=proj, d=6):
        p = [None if x is None else x.ctypes.data for x in (dirs, proj)]
        return c.lib.nerf_sh_radiance_lattice(c.h, which, n, degree, p[0], p[1], d, out.ctypes.data, 0)
    # the bake, in the header's order: each call is wrong in everything after the refusal it meets, too
    assert bake(which=2, n=1, degree=4, d=0) != 0 and "which must be 0 (coarse) or 1 (fine)" in last()
    assert bake(n=1, degree=4, d=0) != 0 and "needs a scene box" in last()
    with pytest.raises(RuntimeError, match="needs a scene box"):
        c.sh_radiance_lattice(0, 3, 1)
    c.set_scene_box(LO, HI)
    for n in (1, 513):
        assert bake(n=n, degree=4, d=0) != 0 and f"n must be in 2..512 (got {n})" in last()
        with pytest.raises(ValueError, match=r"n must be in 2\.\.512"):
            c.sh_radiance_lattice(0, n, 1)
    for degree in (-1, 4):
        assert bake(degree=degree, d=0) != 0 and f"degree must be in 0..3 (got {degree})" in last()
        with pytest.raises(ValueError, match=r"degree must be in 0\.\.3"):
            c.sh_radiance_lattice(0, 3, degree)
    for d in (0, 65):
        assert bake(d=d, dirs=None) != 0 and f"D must be in 1..64 (got {d})" in last()
    with pytest.raises(ValueError, match=r"D in 1\.\.64"):
        c.sh_radiance_lattice(0, 3, 0, dirs=np.ones((65, 3), F), proj=np.ones((1, 65), F))
    assert bake(dirs=None) != 0 and "dirs is NULL" in last()
    assert bake(proj=None) != 0 and "proj is NULL" in last()
    with pytest.raises(ValueError, match="both dirs and proj, or neither"):
        c.sh_radiance_lattice(0, 3, 1, dirs=dirs)
    with pytest.raises(ValueError, match="proj must be"):
        c.sh_radiance_lattice(0, 3, 1, dirs=dirs, proj=proj[:3])
    for bad in (np.nan, np.inf):
        broken = dirs.copy()
        broken[4, 1] = bad
        assert bake(dirs=broken) != 0 and "dirs[4][1] is not finite" in last()
        with pytest.raises(ValueError, match="must be finite"):
            c.sh_radiance_lattice(0, 3, 1, dirs=broken, proj=proj)
        broken = proj.copy()
        broken[2, 5] = bad
        assert bake(proj=broken) != 0 and "proj[2][5] is not finite" in last()
        with pytest.raises(ValueError, match="must be finite"):
            c.sh_radiance_lattice(0, 3, 1, dirs=dirs, proj=broken)
    zero = dirs.copy()
    zero[3] = (0.0, -0.0, 0.0)
    assert bake(dirs=zero) != 0 and "dirs[3] is the zero vector" in last()
    with pytest.raises(ValueError, match=r"dirs\[3\] is the zero vector"):
        c.sh_radiance_lattice(0, 3, 1, dirs=zero, proj=proj)
    assert bake() != 0 and "network 0 has no weights loaded" in last()
    with pytest.raises(RuntimeError, match="no weights loaded"):
        c.sh_radiance_lattice(0, 3, 1)
    c.load_weights(0, N.glorot_blob(0))
    assert bake() == 0 and c.sh_radiance_lattice(0, 2, 3).shape == (2, 2, 2, 52)
    # the volume calls: shape, channels, n, box, n_steps, t_min, outputs
    v = SH.random_sh_volume(3, 1, 40)
    o, d = rays_through_box(4, 41)
    c2w = oracle.get_sphere_matrix(4.0, 0.0, 0.0, 0.0).astype(F)
    for channels in (3, 8, 12, 20, 48, 56):
        with pytest.raises(ValueError, match=r"an SH volume has 4, 16, 28, 52 channels"):
            c.march_sh_volume(np.zeros((3, 3, 3, channels), F), LO, HI, o, d, 4)
    with pytest.raises(ValueError, match=r"SH volume must be an \(n, n, n, C\) array"):
        c.sample_sh_volume(v[:2], LO, HI, o[:, :3], d[:, :3])
    with pytest.raises(ValueError, match=r"n must be in 2\.\.512"):
        c.march_sh_volume(np.zeros((1, 1, 1, 16), F), LO, HI, o, d, 4)
    with pytest.raises(ValueError, match="lo < hi on every axis"):
        c.march_sh_volume(v, LO, (HI[0], LO[1], HI[2]), o, d, 4)
    with pytest.raises(ValueError, match="lo < hi on every axis"):
        c.sample_sh_volume(v, LO, (LO[0] - 1.0, HI[1], HI[2]), o[:, :3], d[:, :3])
    for steps in (0, -3):
        with pytest.raises(ValueError, match="n_steps must be"):
            c.march_sh_volume(v, LO, HI, o, d, steps)
    for t in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError, match=r"t_min must be in \[0, 1\)"):
            c.march_sh_volume(v, LO, HI, o, d, 4, t_min=t)
        with pytest.raises(ValueError, match=r"t_min must be in \[0, 1\)"):
            c.render_sh_volume_image(v, LO, HI, c2w, 0.7, 4, 4, 4, t_min=t)
    # ... and the library's own checks of the same arguments
    lo, hi = np.array(LO, F), np.array(HI, F)
    res = [np.zeros(12, F), np.zeros(4, F), np.zeros(4, F)]

    def march(n=3, degree=1, lo=lo, hi=hi, steps=4, t_min=0.0, outs=res):
        p = [None if x is None else x.ctypes.data for x in outs]
        return c.lib.nerf_sh_volume_march(c.h, v.ctypes.data, n, degree, lo.ctypes.data, hi.ctypes.data, o.ctypes.data,
                                          d.ctypes.data, 4, steps, t_min, p[0], p[1], p[2], 0)
    assert march() == 0
    assert march(outs=[None, res[1], None]) == 0
    assert march(n=1) != 0 and "n must be in 2..512" in last()
    assert march(n=513) != 0 and "n must be in 2..512" in last()
    for degree in (-1, 4):
        assert march(degree=degree) != 0 and f"degree must be in 0..3 (got {degree})" in last()
    assert march(hi=lo) != 0 and "lo < hi on every axis" in last()
    assert march(steps=0) != 0 and "n_steps must be >= 1" in last()
    for t in (-0.1, 1.0, float("nan")):
        assert march(t_min=t) != 0 and "t_min must be in [0, 1)" in last()
    assert march(outs=[None, None, None]) != 0 and "rgb, depth and opacity are all NULL" in last()
    assert c.lib.nerf_sh_volume_render_image(c.h, v.ctypes.data, 3, 1, lo.ctypes.data, hi.ctypes.data, c2w.ctypes.data, 0.7, 4, 4,
                                             0, 0, 4, 0.0, None, None, None, 0) != 0 and "all NULL" in last()
    assert c.lib.nerf_sh_volume_render_image(c.h, v.ctypes.data, 3, 7, lo.ctypes.data, hi.ctypes.data, c2w.ctypes.data, 0.7, 4, 4,
                                             0, 0, 4, 0.0, res[0].ctypes.data, None, None, 0) != 0 and "degree must be" in last()
    pts = np.zeros((4, 3), F)
    assert c.lib.nerf_sh_volume_sample(c.h, v.ctypes.data, 600, 1, lo.ctypes.data, hi.ctypes.data, pts.ctypes.data, pts.ctypes.data,
                                       4, out.ctypes.data, 0) != 0 and "n must be in 2..512" in last()
    assert c.lib.nerf_sh_volume_sample(c.h, v.ctypes.data, 3, 4, lo.ctypes.data, hi.ctypes.data, pts.ctypes.data, pts.ctypes.data,
                                       4, out.ctypes.data, 0) != 0 and "degree must be in 0..3 (got 4)" in last()
    c.close()
    # the model
    rc = {"n_render_samples_coarse": 8, "n_render_samples_fine": 16, "scene_box": [list(LO), list(HI)]}
    m = N.NeRF(S.NET, rc, 2.0, 6.0, precision="fp32")
    with pytest.raises(RuntimeError, match="bake_preview first"):
        m.render_preview(c2w, 0.7, 4, 4)
    with pytest.raises(ValueError, match="cannot be combined with view_dir or camera"):
        m.bake_preview(8, sh_degree=2, camera=c2w)
    with pytest.raises(ValueError, match="cannot be combined with view_dir or camera"):
        m.bake_preview(8, sh_degree=2, view_dir=(0.0, 0.0, 1.0))
    with pytest.raises(ValueError, match="need sh_degree"):
        m.bake_preview(8, sh_dirs=dirs, sh_proj=proj)
    with pytest.raises(ValueError, match=r"degree must be in 0\.\.3"):
        m.bake_preview(8, sh_degree=5)
    with pytest.raises(RuntimeError, match="no weights loaded"):
        m.bake_preview(8, sh_degree=2)
    with pytest.raises(RuntimeError, match="bake_preview first"):
        m.render_preview(c2w, 0.7, 4, 4)
    m.ctx.close()


# ---- 7. the shipped checkpoint ------------------------------------------------------------------------------------------------------
def test_preview_of_the_shipped_checkpoint(golden_ckpt):
    import nerf_and_dietnerf_amd as N
    near, far, fov = float(golden_ckpt["near"]), float(golden_ckpt["far"]), float(golden_ckpt["fov"])
    rc = {"n_render_samples_coarse": 64, "n_render_samples_fine": 128, "scene_box": [list(GOLDEN_BOX[0]), list(GOLDEN_BOX[1])]}
    m = N.NeRF(S.NET, rc, near, far, precision="f16x3")
    m.set_weights(golden_ckpt["blob_coarse"], golden_ckpt["blob_fine"])
    h, w = golden_ckpt["img_test"].shape[:2]
    centre = 0.5 * (np.array(GOLDEN_BOX[0]) + np.array(GOLDEN_BOX[1]))
    poses = {"golden pose": golden_ckpt["c2w_test"].astype(F), "50 degrees away": SH.orbit(golden_ckpt["c2w_test"], centre, 50.0)}
    m.bake_preview(64, sh_degree=2)
    volume, lo, hi, resolution = m._preview
    assert volume.is_cuda and tuple(volume.shape) == (64, 64, 64, 28) and resolution == 64 and (lo, hi) == GOLDEN_BOX
    assert m._preview_sh_degree == 2
    same_f32(m.ctx.sh_radiance_lattice(1, 64, 2), volume.cpu().numpy())        # the fine network, the default table
    sh_frames = {}
    for name, c2w in poses.items():
        rgb, depth, opacity = (x.cpu().numpy() for x in m.render_preview(c2w, fov, h, w))
        assert rgb.shape == (h, w, 3) and depth.shape == (h, w) and opacity.shape == (h, w)
        assert np.isfinite(rgb).all() and np.isfinite(depth).all() and np.isfinite(opacity).all()
        assert opacity.min() >= 0.0 and opacity.max() <= 1.0 and (opacity > 0.5).sum() > 100, name
        assert rgb.min() >= 0.0 and (rgb.max(axis=2) <= opacity + 2 * march_bar(128)).all()
        by_hand = [x.cpu().numpy() for x in m.ctx.render_sh_volume_image(volume, lo, hi, c2w, fov, h, w, 128, 1.0 / 512.0)]
        same_f32(by_hand[0], rgb)
        same_f32(by_hand[2], opacity)
        sh_frames[name] = rgb
    # without the keyword: the plain volume with the bits it always had, marched by the plain march
    m.bake_preview(64)
    volume, lo, hi, resolution = m._preview
    assert tuple(volume.shape) == (64, 64, 64, 4) and m._preview_sh_degree is None
    same_f32(m.ctx.radiance_lattice(1, 64), volume.cpu().numpy())
    c2w = poses["golden pose"]
    plain = m.render_preview(c2w, fov, h, w)
    by_hand = m.ctx.render_volume_image(volume, lo, hi, c2w, fov, h, w, 128, 1.0 / 512.0)
    same_f32(by_hand[0].cpu().numpy(), plain[0].cpu().numpy())
    # printed, not barred: each bake against the network render of the same pose, whole frame / pixels the preview leaves opaque
    def psnr(a, b):
        return float(-10.0 * np.log10(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))
    nets = {name: np.asarray(m.render_image(c2w, fov, h, w, seed=0)[0]).reshape(h, w, 3) for name, c2w in poses.items()}
    bakes = [("constant direction", {}), ("camera at the golden pose", {"camera": poses["golden pose"]})] + \
            [(f"SH degree {degree}", {"sh_degree": degree}) for degree in DEGREES]
    for label, kw in bakes:
        m.bake_preview(64, **kw)
        for name, c2w in poses.items():
            rgb, _, opacity = (x.cpu().numpy() for x in m.render_preview(c2w, fov, h, w))
            if kw.get("sh_degree") == 2:
                same_f32(rgb, sh_frames[name])
            opaque = opacity > 0.99
            print(f"[preview, shipped checkpoint, n = 64, {label}, {name}] PSNR against the network render: "
                  f"{psnr(rgb, nets[name]):.2f} dB whole frame, {psnr(rgb[opaque], nets[name][opaque]):.2f} dB on "
                  f"{int(opaque.sum())} opaque pixels")
    m.ctx.close()
