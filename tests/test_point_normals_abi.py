"""CPU-side checks of the k-NN PCA point normals: csrc/normal_math.h compiled for the host against numpy.linalg.eigh in
float64 on the same neighbourhoods (noisy plane, sphere, cylinder, 7 x 9 wavy grid; k = 3, 5, 16, 64), the conditioning
rule that decides which points enter the comparison, the exact cases (dyadic plane, coincident and collinear points,
canonical sign, viewpoint flip), the stand-alone program, the export of csrc/normals.hip and its argument checks."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests.helpers import native
from tests.helpers.native import ROOT

SOURCE = native.source("normal_math_host.cpp")
NAME = "pn_point_normals_f32"
KS = (3, 5, 16, 64)

# E: the largest angle (radians, up to sign) between the header's normal and numpy.linalg.eigh's over every point of
# every input below that enters the comparison, measured with g++ 13 on x86-64.  It is the rounding of the unit
# vector to fp32 (half an ulp of a component near 1 is 3e-8) — the fp64 eigenvectors themselves agree to 1e-12.
# The bar of every comparison, CPU and GPU, is 4 E: the margin covers another compiler's sqrt and division sequence,
# not another algorithm.
E = 4.6e-8
BAR = 4.0 * E
GAP_MIN = 1e-3        # a point enters the comparison only if the REFERENCE's gap is at least this
LEFT_OUT_MAX = 0.02   # and at most this fraction of an input's points may be left out
# The scalars.  An eigenvalue is a Rayleigh quotient: a unit vector at angle e from the eigenvector of l_i has
# x^T C x = l_i + O(e^2) (l_2 - l_0), so a solver whose vectors are good to E has eigenvalues good to E^2 l_2 (the fp64
# solvers are far better: 1e-16 l_2).  With every |dl_i| <= E^2 l_2 and l_2 <= l_0 + l_1 + l_2 = s:
#   variation = l_0 / s:         |d| <= dl_0 / s + variation * 3 E^2 l_2 / s <= E^2 + 3 E^2 / 3      = 2 E^2
#   gap = (l_1 - l_0) / l_2:     |d| <= 2 E^2 + gap * E^2                                            <= 3 E^2
# on top of the 4 * 2^-24 relative that the single rounding to fp32 (2^-24) is given.
SCALAR_REL = 4.0 * 2.0 ** -24
VARIATION_ABS = 2.0 * E * E
GAP_ABS = 3.0 * E * E


# ---------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------
def plane_patch(seed=3, noise=1e-3, edge=0.05, jitter=0.1):
    """A random planar patch: 300 vertices of a honeycomb of edge 0.05 in a tilted plane, each moved at random by up
    to a tenth of the edge inside the plane and by Gaussian noise 1e-3 across it.  Why a honeycomb and not uniform
    points or a lattice: the two nearest neighbours of a uniform random point are within 6 degrees of a straight line
    through it one time in twenty, and those of a lattice node are opposite nodes; a honeycomb vertex sees its
    neighbours 120 degrees apart, so that the k = 3 normal (the normal of a triangle) is defined at every point."""
    rng = np.random.RandomState(seed)
    i, j = np.meshgrid(np.arange(15), np.arange(10), indexing="ij")
    cell = np.stack([1.5 * i + 1.5 * j * 0, np.sqrt(3.0) * j + np.sqrt(3.0) / 2 * (i % 2)], -1).reshape(-1, 1, 2)
    uv = (cell + np.asarray([[0.0, 0.0], [1.0, 0.0]])).reshape(-1, 2)      # two vertices per cell: 300
    uv = edge * (uv - uv.mean(0) + jitter * rng.uniform(-1, 1, uv.shape))
    a, b = np.asarray([0.8, 0.1, 0.59]), np.asarray([-0.2, 0.9, 0.12])
    a = a / np.linalg.norm(a)
    b = b - (b @ a) * a
    b = b / np.linalg.norm(b)
    nrm = np.cross(a, b)
    return (0.1 + uv[:, :1] * a + uv[:, 1:] * b + noise * rng.standard_normal((uv.shape[0], 1)) * nrm).astype(np.float32)


def sphere(n=500):
    """The unit sphere at 500 points of the golden-angle spiral: three neighbouring points of an even sampling lie on
    a small circle, far from a straight line."""
    i = np.arange(n) + 0.5
    z, phi = 1.0 - 2.0 * i / n, np.pi * (3.0 - np.sqrt(5.0)) * i
    r = np.sqrt(1.0 - z * z)
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], 1).astype(np.float32)


def cylinder(n=353, seed=5, radius=0.3, noise=0.0):
    """Axis (1,2,2)/3 through (0.1,-0.2,0.05).  Returns the points and the analytic (outward) normals."""
    rng = np.random.RandomState(seed)
    axis = np.asarray([1.0, 2.0, 2.0]) / 3.0
    u = np.cross(axis, [1.0, 0.0, 0.0])
    u /= np.linalg.norm(u)
    v = np.cross(axis, u)
    th, h = rng.uniform(0, 2 * np.pi, n), rng.uniform(-0.5, 0.5, n)
    radial = np.cos(th)[:, None] * u + np.sin(th)[:, None] * v
    pts = np.asarray([0.1, -0.2, 0.05]) + h[:, None] * axis + (radius + noise * rng.standard_normal(n))[:, None] * radial
    return pts.astype(np.float32), radial.astype(np.float32)


def wavy_grid(U=7, V=9, seed=0):
    """The 7 x 9 grid, its nodes shifted along the rows by +-0.02 in a checkerboard: on the bare lattice the two
    nearest neighbours of a node are the two next nodes of its row, three collinear points, and the k = 3 normal is
    undefined everywhere."""
    rng = np.random.RandomState(seed)
    i, j = np.meshgrid(np.arange(U), np.arange(V), indexing="ij")
    u = np.linspace(-0.4, 0.4, U)[i] + 0.02 * (1 - 2 * ((i + j) % 2))
    v = np.linspace(-0.45, 0.45, V)[j]
    z = 0.1 * np.sin(5 * u) * np.cos(4 * v) + 0.01 * rng.standard_normal(u.shape)
    return np.stack([u, v, z], 2).reshape(-1, 3).astype(np.float32)


def inputs():
    return {"plane, noise 1e-3": plane_patch(), "sphere 500": sphere(), "cylinder": cylinder()[0],
            "wavy 7x9 grid": wavy_grid()}


# ---------------------------------------------------------------------------------------------
# the float64 restatement
# ---------------------------------------------------------------------------------------------
def knn3(P, k):
    """(n,k) int32 neighbours by knn3's rule: d = ((dx^2 + dy^2) + dz^2) in fp32, nearest first, equal distances to
    the smaller index, a cloud of fewer than k points padded with the point itself."""
    P = np.asarray(P, np.float32)
    n = P.shape[0]
    d = P[:, None, :] - P[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    assert d2.dtype == np.float32
    order = np.argsort(d2, axis=1, kind="stable").astype(np.int32)
    if n >= k:
        return np.ascontiguousarray(order[:, :k])
    return np.ascontiguousarray(np.concatenate([order, np.repeat(np.arange(n, dtype=np.int32)[:, None], k - n, 1)], 1))


def reference(P, idx):
    """numpy.linalg.eigh on the float64 covariance of every neighbourhood: (normals (n,3), variation, gap, eigenvalues
    (n,3) ascending), all float64; degenerate rows (l2 <= 1e-30, fewer than 3 points) are zero."""
    P = np.asarray(P, np.float32).astype(np.float64)
    n, k = idx.shape
    nb = P[idx]                                              # (n,k,3)
    d = nb - nb.mean(1, keepdims=True)
    C = np.einsum("nka,nkb->nab", d, d) / k
    w, v = np.linalg.eigh(C)
    w = np.maximum(w, 0.0)
    live = (w[:, 2] > 1e-30) & (n >= 3)
    safe = np.where(live, w[:, 2], 1.0)
    nrm = np.where(live[:, None], v[:, :, 0], 0.0)
    variation = np.where(live, w[:, 0] / np.where(live, w.sum(1), 1.0), 0.0)
    gap = np.where(live, (w[:, 1] - w[:, 0]) / safe, 0.0)
    return nrm, variation, gap, w


def angle(a, b):
    """Angle between the lines spanned by the rows of a and b (so up to sign), float64, exact for small angles."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), np.abs((a * b).sum(1)))


def segment_reference(clouds, k):
    """The restatement over a ragged batch: (flat points, off, idx, normals, variation, gap)."""
    off = np.concatenate([[0], np.cumsum([c.shape[0] for c in clouds])]).astype(np.int32)
    parts = [(knn3(c, k),) + reference(c, knn3(c, k))[:3] if c.shape[0] else
             (np.zeros((0, k), np.int32), np.zeros((0, 3)), np.zeros(0), np.zeros(0)) for c in clouds]
    cat = [np.concatenate([p[i] for p in parts]) for i in range(4)]
    return np.concatenate(clouds).astype(np.float32), off, cat[0], cat[1], cat[2], cat[3]


# ---------------------------------------------------------------------------------------------
# the host-compiled header
# ---------------------------------------------------------------------------------------------
def build_harness(directory):
    lib = native.build_harness(directory, "nmh", SOURCE)
    lib.nmh_sweeps.restype = ctypes.c_int
    return lib


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory.mktemp("nmh"))


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def header(harness, P, off, idx, view=None, sweeps=None):
    """(normals (total,3), variation, gap) fp32 of the host-compiled header over a ragged batch."""
    P, off, idx = np.ascontiguousarray(P, np.float32), np.ascontiguousarray(off, np.int32), np.ascontiguousarray(idx, np.int32)
    view = None if view is None else np.ascontiguousarray(view, np.float32)
    total, k = idx.shape
    nrm = np.full((total, 3), np.nan, np.float32)
    var, gap = np.full(total, np.nan, np.float32), np.full(total, np.nan, np.float32)
    harness.nmh_normals(_p(P), _p(off), off.shape[0] - 1, _p(idx), k, harness.nmh_sweeps() if sweeps is None else sweeps,
                        _p(view), _p(nrm), _p(var), _p(gap))
    return nrm, var, gap


def header_cloud(harness, P, k, **kw):
    return header(harness, P, np.asarray([0, P.shape[0]], np.int32), knn3(P, k), **kw)


def check_against_reference(got, want, what, bar=BAR):
    """got: (normals, variation, gap) fp32; want: the restatement's.  Asserts the bars, returns the largest angle."""
    (n_g, v_g, g_g), (n_r, v_r, g_r) = got, want
    assert np.isfinite(n_g).all() and np.isfinite(v_g).all() and np.isfinite(g_g).all(), what
    dead = ~n_r.any(1)
    assert not n_g[dead].any() and not v_g[dead].any() and not g_g[dead].any(), what
    length = np.linalg.norm(n_g[~dead].astype(np.float64), axis=1)
    assert np.abs(length - 1.0).max(initial=0.0) <= 4 * 2.0 ** -24, what
    assert (np.abs(v_g - v_r) <= VARIATION_ABS + SCALAR_REL * np.abs(v_r)).all(), what
    assert (np.abs(g_g - g_r) <= GAP_ABS + SCALAR_REL * np.abs(g_r)).all(), what
    enters = ~dead & (g_r >= GAP_MIN)
    worst = float(angle(n_g[enters], n_r[enters]).max(initial=0.0))
    assert worst <= bar, (what, worst, bar)
    return worst, int(enters.sum())


def test_the_reference_leaves_out_at_most_two_percent():
    """The conditioning rule: an eigenvector is defined to about |dC| / (l1 - l0), so a point enters the comparison
    only if the reference's own gap >= 1e-3 — and every input keeps at least 98 % of its points at every k."""
    for name, P in inputs().items():
        for k in KS:
            _, _, gap, _ = reference(P, knn3(P, k))
            out = float((gap < GAP_MIN).mean())
            print("%s, k = %d: %.2f %% of %d points below gap %g" % (name, k, 100 * out, P.shape[0], GAP_MIN))
            assert out <= LEFT_OUT_MAX, (name, k, out)


def test_header_against_numpy_eigh(harness):
    """Measured here: E = 4.6e-8 rad (bar 1.84e-7): the largest angle over the 4 864 neighbourhoods (4 inputs x 4 k)."""
    worst = 0.0
    for name, P in inputs().items():
        for k in KS:
            idx = knn3(P, k)
            e, m = check_against_reference(header_cloud(harness, P, k), reference(P, idx)[:3], (name, k))
            print("%s, k = %d: %d of %d points compared, largest angle %.3e (E %.1e, bar %.1e)"
                  % (name, k, m, P.shape[0], e, E, BAR))
            worst = max(worst, e)
    print("largest angle over all inputs: %.3e" % worst)
    assert 0 < worst <= BAR


def test_one_sweep_fewer_gives_the_same_bits(harness):
    """NM_SWEEPS is the smallest number of sweeps after which one more changes no output bit on these inputs, plus
    one: so NM_SWEEPS - 1 and NM_SWEEPS, and one more, agree in every bit."""
    s = harness.nmh_sweeps()
    assert s == 5
    for name, P in inputs().items():
        for k in KS:
            base = header_cloud(harness, P, k)
            for other in (s - 1, s + 1):
                got = header_cloud(harness, P, k, sweeps=other)
                assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(base, got)), (name, k)


# ---------------------------------------------------------------------------------------------
# exact cases
# ---------------------------------------------------------------------------------------------
def _dyadic_plane(n=40, seed=11, c=0.375):
    rng = np.random.RandomState(seed)
    xy = rng.randint(-64, 64, (n, 2)) / 128.0
    return np.concatenate([xy, np.full((n, 1), c)], 1).astype(np.float32)


def test_a_dyadic_plane_has_exactly_the_z_normal(harness):
    P = _dyadic_plane()
    for k in (5, 16, 64):
        nrm, var, gap = header_cloud(harness, P, k)
        assert np.array_equal(nrm, np.tile(np.asarray([0, 0, 1], np.float32), (P.shape[0], 1))), k
        assert not var.any() and (gap > 0).all()
    # seen from below the plane every normal points down, exactly
    nrm, _, _ = header_cloud(harness, P, 16, view=np.asarray([[0.0, 0.0, -1.0]], np.float32))
    assert np.array_equal(nrm, np.tile(np.asarray([0, 0, -1], np.float32), (P.shape[0], 1)))


def test_coincident_points_give_the_zero_normal(harness):
    P = np.tile(np.asarray([[0.3, -0.7, 0.11]], np.float32), (9, 1))
    for k in (3, 9, 16):
        for view in (None, np.asarray([[1.0, 2.0, 3.0]], np.float32)):
            nrm, var, gap = header_cloud(harness, P, k, view=view)
            assert not nrm.any() and not var.any() and not gap.any()
            assert not np.signbit(nrm).any()
    # fewer than three points: zero, whatever they are; three distinct points: a normal
    for n in (1, 2):
        nrm, var, gap = header_cloud(harness, _dyadic_plane()[:n], 3)
        assert not nrm.any() and not var.any() and not gap.any()
    assert header_cloud(harness, _dyadic_plane()[:3], 3)[0].any(1).all()


def test_collinear_points_are_finite_with_no_gap(harness):
    t = np.arange(12, dtype=np.float64)[:, None]
    for direction in ([1.0, 0.0, 0.0], [0.25, -0.5, 0.125], [0.3, 0.7, -0.2]):
        P = (np.asarray([0.1, 0.2, 0.3]) + 0.05 * t * np.asarray(direction)).astype(np.float32)
        for k in (3, 5, 12):
            nrm, var, gap = header_cloud(harness, P, k)
            assert np.isfinite(nrm).all() and np.isfinite(var).all() and np.isfinite(gap).all()
            assert (gap >= 0).all() and (gap < 1e-6).all() and (var >= 0).all() and (var < 1e-6).all()
            assert np.abs(np.linalg.norm(nrm.astype(np.float64), axis=1) - 1).max() <= 4 * 2.0 ** -24
            # the normal of a line is any direction across it
            across = np.abs(nrm.astype(np.float64) @ (np.asarray(direction) / np.linalg.norm(direction)))
            assert across.max() < 1e-6


def _canonical(harness, n):
    n = np.asarray(n, np.float32).copy()
    harness.nmh_canonical(_p(n))
    return n.tolist()


def test_canonical_sign(harness):
    assert _canonical(harness, [-0.5, 0.25, 0.25]) == [0.5, -0.25, -0.25]
    assert _canonical(harness, [0.25, -0.5, 0.25]) == [-0.25, 0.5, -0.25]
    assert _canonical(harness, [0.25, 0.25, -0.5]) == [-0.25, -0.25, 0.5]
    assert _canonical(harness, [0.5, -0.25, 0.25]) == [0.5, -0.25, 0.25]
    # ties of the two (three) largest magnitudes: the lowest axis decides
    assert _canonical(harness, [-0.5, 0.5, 0.0]) == [0.5, -0.5, 0.0]
    assert _canonical(harness, [0.5, -0.5, 0.0]) == [0.5, -0.5, 0.0]
    assert _canonical(harness, [0.0, -0.5, 0.5]) == [0.0, 0.5, -0.5]
    assert _canonical(harness, [-0.5, 0.0, 0.5]) == [0.5, 0.0, -0.5]
    assert _canonical(harness, [-0.5, -0.5, 0.5]) == [0.5, 0.5, -0.5]
    assert _canonical(harness, [0.0, 0.0, 0.0]) == [0.0, 0.0, 0.0]
    # a whole neighbourhood: the plane x = y, whose normal (1,-1,0) / sqrt 2 ties in its two largest magnitudes
    rng = np.random.RandomState(2)
    a, z = rng.randint(-64, 64, 30) / 128.0, rng.randint(-64, 64, 30) / 128.0
    nrm, _, _ = header_cloud(harness, np.stack([a, a, z], 1).astype(np.float32), 8)
    assert (nrm[:, 0] == -nrm[:, 1]).all() and (nrm[:, 0] > 0.7).all() and not nrm[:, 2].any()
    # and on every input: the first component of largest magnitude is positive
    for name, P in inputs().items():
        nrm, _, _ = header_cloud(harness, P, 16)
        lead = nrm[np.arange(nrm.shape[0]), np.argmax(np.abs(nrm), 1)]
        assert (lead > 0).all(), name


def _orient(harness, n, p, v):
    n = np.asarray(n, np.float32).copy()
    harness.nmh_orient(_p(n), _p(np.asarray(p, np.float32)), _p(np.asarray(v, np.float32)))
    return n.tolist()


def test_viewpoint_flip(harness):
    assert _orient(harness, [0, 0, 1], [0, 0, 0], [0, 0, 2]) == [0, 0, 1]
    assert _orient(harness, [0, 0, 1], [0, 0, 0], [5, 5, -0.25]) == [0, 0, -1]
    assert _orient(harness, [0, 0, 1], [0, 0, 3], [0, 0, 2]) == [0, 0, -1]            # v - p, not v
    assert _orient(harness, [0, 0, 1], [1, 1, 0.5], [4, -2, 0.5]) == [0, 0, 1]        # n . (v - p) == 0: kept
    assert _orient(harness, [0.5, -0.5, 0], [0, 0, 0], [1, 1, 7]) == [0.5, -0.5, 0]   # == 0 by cancellation: kept
    # the dot product is taken in fp64 from the fp32 values: v - p = 1 - 2^-30 rounds to 1 in fp32, where the dot is 0
    assert _orient(harness, [1, -1, 0], [2.0 ** -30, 0, 0], [1, 1, 0]) == [-1, 1, 0]
    assert _orient(harness, [1, -1, 0], [-2.0 ** -30, 0, 0], [1, 1, 0]) == [1, -1, 0]
    for name, P in inputs().items():
        view = np.asarray([[0.3, -0.2, 2.5]], np.float32)
        plain, _, _ = header_cloud(harness, P, 16)
        seen, _, _ = header_cloud(harness, P, 16, view=view)
        dot = (plain.astype(np.float64) * (view.astype(np.float64) - P.astype(np.float64))).sum(1)
        assert (dot != 0).all()
        assert np.array_equal(seen, np.where((dot < 0)[:, None], -plain, plain)), name


def test_the_program_reads_neighbourhoods_from_stdin_and_a_file(harness, tmp_path):
    exe = native.build_program(tmp_path, "normal_math_host", SOURCE)
    P, k = wavy_grid(), 5
    idx = knn3(P, k)
    text = "%d %d\n" % (P.shape[0], k) + "".join("%.9g %.9g %.9g\n" % tuple(p) for p in P)
    text += "".join(" ".join(str(j) for j in row) + "\n" for row in idx)
    path = tmp_path / "grid.txt"
    path.write_text(text)
    want = np.concatenate([a.reshape(P.shape[0], -1) for a in header_cloud(harness, P, k)], 1)
    for run in (subprocess.run([exe], input=text, capture_output=True, text=True, check=True),
                subprocess.run([exe, str(path)], capture_output=True, text=True, check=True)):
        got = np.asarray([[float(x) for x in line.split()] for line in run.stdout.splitlines()], np.float32)
        assert np.array_equal(got, want)
    assert subprocess.run([exe], input="5 2\n", capture_output=True, text=True).returncode == 2


# ---------------------------------------------------------------------------------------------
# the export and the argument checks, which run before anything touches a GPU
# ---------------------------------------------------------------------------------------------
def load_raw():
    return native.load_raw((NAME, "pn_point_normals_tile"))


@pytest.fixture(scope="module")
def lib():
    return load_raw()


def test_the_entry_point_is_exported_and_bound(lib):
    from parsenet_codebase_amd import _lib
    v, i = ctypes.c_void_p, ctypes.c_int
    assert _lib.SIGNATURES[NAME] == (i, [v, v, i, i, v, i, v, v, v, i, v, v, v, v])
    assert _lib.SIGNATURES["pn_point_normals_tile"] == (i, [])
    assert lib.pn_point_normals_tile() == 64
    assert [line for line in open(os.path.join(ROOT, "include", "parsenet_hip.h")) if NAME + "(" in line]


def raw_call(lib, **over):
    """pn_point_normals_f32 with plausible arguments (never dereferenced by a call that is refused), some replaced."""
    a = dict(pts=64, off=64, S=1, total=10, idx=64, k=8, viewpoints=None, tile_seg=64, tile_first=64, total_tiles=1,
             normals=64, variation=None, gap=None, stream=None)
    a.update(over)
    return lib.pn_point_normals_f32(*[a[n] for n in ("pts", "off", "S", "total", "idx", "k", "viewpoints", "tile_seg",
                                                      "tile_first", "total_tiles", "normals", "variation", "gap", "stream")])


def check_invalid_arguments(lib, **real):
    """k out of range, S < 0, a null required pointer: PN_ERR_ARG; nothing to do: 0."""
    from parsenet_codebase_amd import _lib
    err = _lib.CONSTANTS["PN_ERR_ARG"]
    for over in (dict(k=2), dict(k=65), dict(k=0), dict(S=-1), dict(total=-1), dict(pts=None), dict(off=None),
                 dict(idx=None), dict(normals=None), dict(tile_seg=None), dict(tile_first=None), dict(total_tiles=0)):
        assert raw_call(lib, **dict(real, **over)) == err, over
        assert b"pn_point_normals_f32" in lib.pn_last_error()
    assert raw_call(lib, **dict(real, total=0)) == 0
    assert raw_call(lib, **dict(real, S=0)) == 0
    assert raw_call(lib, **dict(real, total=0, pts=None, idx=None, normals=None, total_tiles=0)) == 0


def test_invalid_arguments_are_refused_before_any_launch(lib):
    """(No GPU is needed to get here: a refused call, and one with nothing to do, launch nothing.)"""
    check_invalid_arguments(lib)


def test_python_argument_checks_need_no_gpu():
    import torch
    from parsenet_codebase_amd import kernels, point_normals
    with pytest.raises(RuntimeError, match="MI355X only"):
        point_normals.estimate_normals(torch.zeros(8, 3))
    with pytest.raises(RuntimeError, match="MI355X only"):
        kernels.point_normals(torch.zeros(8, 3), [0, 8], torch.zeros(8, 3, dtype=torch.int32), 3)
    with pytest.raises(TypeError):
        point_normals.estimate_normals(np.zeros((8, 3), np.float32))
    with pytest.raises(ValueError, match="empty list"):
        point_normals.estimate_normals([])
