"""numpy float32 restatement of the isosurface rule of include/nerf_mi355.h (nerf_isosurface): marching tetrahedra on the
6-tetrahedra Kuhn split of every cube, vertices numbered by (lattice point, edge type), triangles by (cube, tetrahedron).
Every float32 operation is rounded on its own, as the kernels' __f*_rn arithmetic is, so the device result can be compared
bit for bit.

The orientation of every polygon is decided HERE from geometry that cannot degenerate -- the midpoints of the crossed edges
in lattice coordinates, against (centroid of the outside corners - centroid of the inside corners) -- and not from the
kernels' case table, which is what this file checks.

A volume is an (n, n, n) array indexed [iz, iy, ix]: lattice point (ix, iy, iz) is element ix + n (iy + n iz)."""
import itertools

import numpy as np

F = np.float32
EDGE_TYPES = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1), (1, 1, 1))     # (dx, dy, dz), in key order
TYPE_OF = {e: t for t, e in enumerate(EDGE_TYPES)}
PERMS = tuple(itertools.permutations(range(3)))                                               # lexicographic: 012 ... 210


def tet_corners(perm):
    """The four corners of the tetrahedron of axis permutation (a, b, c), as (dx, dy, dz) offsets from the cube's base."""
    c = [np.zeros(3, int)]
    for ax in perm:
        nxt = c[-1].copy()
        nxt[ax] += 1
        c.append(nxt)
    return c


def _polygon(inside4):
    """Corner pairs (i, j), i < j, of the crossed edges in the rule's order, before orientation."""
    k = sum(inside4)
    if k in (1, 3):
        odd = [i for i in range(4) if inside4[i] == (k == 1)][0]
        return [(min(odd, j), max(odd, j)) for j in range(4) if j != odd]
    if k == 2:
        i0, i1 = [i for i in range(4) if inside4[i]]
        o0, o1 = [i for i in range(4) if not inside4[i]]
        return [tuple(sorted(p)) for p in ((i0, o0), (i0, o1), (i1, o1), (i1, o0))]
    return []


def _oriented_cases():
    """table[perm][case] -> the polygon's corner pairs, counter-clockwise seen from the outside; case bit i = corner i inside."""
    table = []
    for perm in PERMS:
        c = [x.astype(np.float64) for x in tet_corners(perm)]
        row = []
        for case in range(16):
            ins = [bool(case >> i & 1) for i in range(4)]
            poly = _polygon(ins)
            if poly:
                mid = [(c[i] + c[j]) / 2 for i, j in poly]
                normal = sum(np.cross(mid[q], mid[(q + 1) % len(mid)]) for q in range(len(mid)))      # Newell
                out = np.mean([c[i] for i in range(4) if not ins[i]], axis=0) - np.mean([c[i] for i in range(4) if ins[i]], axis=0)
                d = float(normal @ out)
                assert abs(d) > 1e-9
                if d < 0:
                    poly = poly[::-1]
            row.append(poly)
        table.append(row)
    return table


CASES = _oriented_cases()


def lattice_step(lo, hi, n):
    return (np.asarray(hi, F) - np.asarray(lo, F)) / F(n - 1)


def lattice_points(lo, hi, n):
    """(n^3, 3) float32 positions lo + step * float(i), in element order (x fastest)."""
    lo = np.asarray(lo, F)
    step = lattice_step(lo, hi, n)
    i = np.arange(n, dtype=F)
    ax = [lo[a] + step[a] * i for a in range(3)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1).astype(F)


def gradients(s, step):
    """(3, m, m, m): per axis x, y, z the central difference over 2 step, one-sided over step at the faces."""
    out = []
    with np.errstate(all="ignore"):
        for a, axis in ((0, 2), (1, 1), (2, 0)):
            sm = np.moveaxis(s, axis, 0)
            g = np.empty_like(sm)
            g[1:-1] = (sm[2:] - sm[:-2]) / (F(2) * step[a])
            g[0] = (sm[1] - sm[0]) / step[a]
            g[-1] = (sm[-1] - sm[-2]) / step[a]
            out.append(np.moveaxis(g, 0, axis))
    return np.stack(out)


def isosurface(s, lo, hi, iso, n=None, offset=(0, 0, 0)):
    """-> vertices (V, 3) float32, normals (V, 3) float32, triangles (T, 3) int32.  ``s`` is the whole (n, n, n) volume, or
    an (m, m, m) block of an n^3 lattice whose first point is lattice point ``offset`` = (ox, oy, oz): positions then are
    those of the whole lattice, and the numbering is the block's own."""
    s = np.ascontiguousarray(s, F)
    m = s.shape[0]
    assert s.shape == (m, m, m) and m >= 2
    n = m if n is None else n
    lo, iso = np.asarray(lo, F), F(iso)
    step = lattice_step(lo, hi, n)
    ins = s > iso                                            # NaN: outside
    grad = gradients(s, step)
    pidx = np.arange(m ** 3, dtype=np.int64).reshape(m, m, m)

    keys, x0, d = [], [], []
    for t, (dx, dy, dz) in enumerate(EDGE_TYPES):
        act = ins[:m - dz, :m - dy, :m - dx] != ins[dz:, dy:, dx:]
        z, y, x = np.nonzero(act)
        keys.append(7 * pidx[z, y, x] + t)
        x0.append(np.stack([x, y, z], axis=1))
        d.append(np.tile(np.array([dx, dy, dz]), (len(x), 1)))
    keys, x0, d = np.concatenate(keys), np.concatenate(x0), np.concatenate(d)
    order = np.argsort(keys, kind="stable")
    keys, x0, d = keys[order], x0[order], d[order]
    x1 = x0 + d
    s0, s1 = s[x0[:, 2], x0[:, 1], x0[:, 0]], s[x1[:, 2], x1[:, 1], x1[:, 0]]
    with np.errstate(all="ignore"):
        t = (iso - s0) / (s1 - s0)
        t = np.where(np.isfinite(t), t, F(0.5)).astype(F)
        off = np.asarray(offset)
        vertices = np.empty((len(keys), 3), F)
        g = np.empty((len(keys), 3), F)
        for a in range(3):
            p0 = lo[a] + step[a] * (x0[:, a] + off[a]).astype(F)
            p1 = lo[a] + step[a] * (x1[:, a] + off[a]).astype(F)
            vertices[:, a] = p0 + t * (p1 - p0)
            g0, g1 = grad[a][x0[:, 2], x0[:, 1], x0[:, 0]], grad[a][x1[:, 2], x1[:, 1], x1[:, 0]]
            g[:, a] = g0 + t * (g1 - g0)
        length = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
        ok = np.isfinite(length) & (length > 0)
        normals = np.where(ok[:, None], -(g / length[:, None]), F(0)).astype(F)

    tris, tri_key = [], []
    cz, cy, cx = np.meshgrid(np.arange(m - 1), np.arange(m - 1), np.arange(m - 1), indexing="ij")
    cube = (cx + (m - 1) * (cy + (m - 1) * cz)).ravel()
    base = np.stack([cx.ravel(), cy.ravel(), cz.ravel()], axis=1)
    for pi, perm in enumerate(PERMS):
        corners = [base + c for c in tet_corners(perm)]
        case = sum(ins[c[:, 2], c[:, 1], c[:, 0]].astype(int) << i for i, c in enumerate(corners))
        for cs in range(1, 15):
            sel = np.nonzero(case == cs)[0]
            if not len(sel):
                continue
            poly = []
            for i, j in CASES[pi][cs]:
                p, e = corners[i][sel], tuple(tet_corners(perm)[j] - tet_corners(perm)[i])
                key = 7 * pidx[p[:, 2], p[:, 1], p[:, 0]] + TYPE_OF[e]
                vid = np.searchsorted(keys, key)
                assert (keys[vid] == key).all()
                poly.append(vid)
            poly = np.stack(poly, axis=1)
            k = poly.shape[1]
            rot = (np.argmin(poly, axis=1)[:, None] + np.arange(k)) % k
            poly = np.take_along_axis(poly, rot, axis=1)
            tris.append(poly[:, [0, 1, 2]])
            tri_key.append((cube[sel] * 6 + pi) * 2)
            if k == 4:
                tris.append(poly[:, [0, 2, 3]])
                tri_key.append((cube[sel] * 6 + pi) * 2 + 1)
    if tris:
        tris, tri_key = np.concatenate(tris), np.concatenate(tri_key)
        triangles = tris[np.argsort(tri_key, kind="stable")].astype(np.int32)
    else:
        triangles = np.zeros((0, 3), np.int32)
    return vertices, normals, triangles


# ---- mesh checks --------------------------------------------------------------------------------------------------------------
def directed_edges(triangles):
    t = np.asarray(triangles, np.int64)
    return np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])


def unmatched_edges(triangles):
    """The directed edges (a, b) that do not occur exactly once with (b, a) occurring exactly once: empty for a closed,
    consistently oriented surface."""
    e = directed_edges(triangles)
    if not len(e):
        return e
    big = int(e.max()) + 1
    code, rev = e[:, 0] * big + e[:, 1], e[:, 1] * big + e[:, 0]
    uniq, counts = np.unique(code, return_counts=True)
    count_of = dict(zip(uniq.tolist(), counts.tolist()))
    bad = np.array([count_of[c] != 1 or count_of.get(r, 0) != 1 for c, r in zip(code.tolist(), rev.tolist())])
    return e[bad]


def euler_characteristic(n_vertices, triangles):
    e = np.sort(directed_edges(triangles), axis=1)
    return n_vertices - len(np.unique(e, axis=0)) + len(triangles)


def signed_volume(vertices, triangles):
    v = np.asarray(vertices, np.float64)
    a, b, c = v[triangles[:, 0]], v[triangles[:, 1]], v[triangles[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def area(vertices, triangles):
    v = np.asarray(vertices, np.float64)
    a, b, c = v[triangles[:, 0]], v[triangles[:, 1]], v[triangles[:, 2]]
    return float(np.linalg.norm(np.cross(b - a, c - a), axis=1).sum() / 2.0)


# ---- the fields of the tests ---------------------------------------------------------------------------------------------------
LO, HI = (-1.0, -1.2, -0.9), (1.1, 1.0, 1.3)
BALL_R, BALL_C = 0.7, (0.05, -0.1, 0.2)


def _xyz(n, lo=LO, hi=HI):
    p = lattice_points(lo, hi, n).astype(np.float64)
    return p[:, 0].reshape(n, n, n), p[:, 1].reshape(n, n, n), p[:, 2].reshape(n, n, n)


def ball(n, r=BALL_R, c=BALL_C):
    x, y, z = _xyz(n)
    return (r - np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2)).astype(F)


def torus(n, big=0.6, small=0.22, z0=0.2):
    x, y, z = _xyz(n)
    return (small - np.sqrt((np.sqrt(x * x + y * y) - big) ** 2 + (z - z0) ** 2)).astype(F)


def two_balls(n):
    return np.maximum(ball(n, 0.35, (-0.4, 0.0, 0.0)), ball(n, 0.3, (0.5, 0.0, 0.3)))


def padded(core, value=-1.0):
    return np.pad(np.asarray(core, F), 1, constant_values=F(value))


def random_field(n, seed):
    """Standard normal values on an n^3 core, inside one layer of -1: (n + 2)^3."""
    return padded(np.random.default_rng(seed).standard_normal((n, n, n)).astype(F))


def tie_field(n=9, seed=3):
    """Integers in {-1, 0, 1}, padded with -1: with iso = 0 many lattice values EQUAL iso, so vertices coincide."""
    return padded(np.random.default_rng(seed).integers(-1, 2, (n, n, n)).astype(F))
