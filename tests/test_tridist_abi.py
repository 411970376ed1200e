"""CPU-side checks of the exact point-to-trimmed-surface distance: csrc/tri_math.h compiled for the host against an
independent float64 restatement (random, grid, sphere-with-poles, hand-placed and exactly degenerate triangles), the
certified bounds against the float64 distances, the exports of csrc/tridist.hip at ABI 23, the header / ctypes table,
and the argument checks of surface.point_surface_distance that need no GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "parsenet_hip.h")
NAMES = ["pn_trimesh_records_f32", "pn_trimesh_point_dist_f32", "pn_trimesh_point_dist_tile", "pn_trimesh_group"]


# ---------------------------------------------------------------------------------------------
# the oracle: min of the three point-to-segment distances and, if the projection onto the plane falls inside the
# triangle, the plane distance; zero-length segments are points.  Generic in the dtype.
# ---------------------------------------------------------------------------------------------
def _segment(P, a, b):
    e = b - a                                                   # (m,3)
    ee = (e * e).sum(-1)
    ap = P[:, None, :] - a[None]                                # (n,m,3)
    live = ee > 0
    t = np.where(live, (ap * e[None]).sum(-1) / np.where(live, ee, 1), 0)
    t = np.clip(t, 0, 1).astype(P.dtype)
    r = ap - t[..., None] * e[None]
    return np.sqrt((r * r).sum(-1))


def oracle(P, tri, dtype=np.float64):
    """(n,m) distances from points P (n,3) to triangles tri (m,3,3)."""
    P = np.asarray(P, dtype)
    a, b, c = (np.asarray(tri[:, k], dtype) for k in range(3))
    d = np.minimum(np.minimum(_segment(P, a, b), _segment(P, b, c)), _segment(P, c, a))
    n = np.cross(b - a, c - a)
    nn = (n * n).sum(-1)
    flat = nn > 0
    unit = (n / np.sqrt(np.where(flat, nn, 1))[:, None]).astype(dtype)
    h = ((P[:, None, :] - a[None]) * unit[None]).sum(-1)        # signed plane distance
    q = P[:, None, :] - h[..., None] * unit[None]               # the projection
    inside = np.broadcast_to(flat[None], h.shape).copy()
    for s, e in ((a, b), (b, c), (c, a)):
        inside &= (np.cross(np.broadcast_to((e - s)[None], q.shape), q - s[None]) * unit[None]).sum(-1) >= 0
    return np.where(inside, np.minimum(d, np.abs(h)), d).astype(dtype)


def grid_triangles(grid, mask=None):
    """(T,3,3) triangles of a (U,V,3) grid in TrimmedSurface.triangles() order."""
    U, V = grid.shape[:2]
    mask = np.ones((U - 1, V - 1), bool) if mask is None else mask
    i, j = np.nonzero(mask)
    g = grid
    return np.stack([np.stack([g[i, j], g[i + 1, j], g[i + 1, j + 1]], 1),
                     np.stack([g[i, j], g[i + 1, j + 1], g[i, j + 1]], 1)], 1).reshape(-1, 3, 3)


def wavy_grid(U=7, V=9, seed=0):
    rng = np.random.RandomState(seed)
    u, v = np.meshgrid(np.linspace(-0.4, 0.4, U), np.linspace(-0.45, 0.45, V), indexing="ij")
    z = 0.1 * np.sin(5 * u) * np.cos(4 * v) + 0.01 * rng.standard_normal(u.shape)
    return np.stack([u, v, z], 2).astype(np.float32)


def sphere_grid(U=7, V=9, radius=0.4):
    """Latitude rows from pole to pole: the first and the last row are U copies of one point (zero-area triangles
    with two equal vertices), the last longitude closes the circle."""
    lam = np.linspace(-1.0, 1.0, U)
    th = np.concatenate([np.arange(V - 1) * 2 * np.pi / (V - 1), np.zeros(1)])
    rad = radius * np.sqrt(np.maximum(1 - lam ** 2, 0.0))
    g = np.stack([rad[:, None] * np.cos(th)[None], rad[:, None] * np.sin(th)[None],
                  np.broadcast_to(radius * lam[:, None], (U, V))], 2)
    g[0, :, :2] = 0.0
    g[-1, :, :2] = 0.0
    return g.astype(np.float32)


def random_triangles(n, seed):
    """Vertices uniform in the cube, kept when the height over the longest edge is at least a tenth of it."""
    rng = np.random.RandomState(seed)
    out = []
    while len(out) < n:
        t = rng.uniform(-0.5, 0.5, (3, 3)).astype(np.float32).astype(np.float64)
        edges = [np.linalg.norm(t[k] - t[(k + 1) % 3]) for k in range(3)]
        area2 = np.linalg.norm(np.cross(t[1] - t[0], t[2] - t[0]))
        if area2 / max(edges) ** 2 >= 0.1:
            out.append(t.astype(np.float32))
    return np.stack(out)


# one triangle and a point in each of its seven regions (face, three edges, three vertices), above the plane
HAND_TRI = np.asarray([[[0.0, 0.0, 0.0], [0.25, 0.0, 0.0], [0.0, 0.25, 0.0]]], np.float32)
HAND_PTS = np.asarray([[0.0625, 0.0625, 0.125],      # face
                       [0.125, -0.125, 0.0625],      # edge ab
                       [0.25, 0.25, 0.0625],         # edge bc
                       [-0.125, 0.125, 0.0625],      # edge ca
                       [-0.125, -0.125, 0.0625],     # vertex a
                       [0.5, -0.0625, 0.0625],       # vertex b
                       [-0.0625, 0.5, 0.0625],       # vertex c
                       [0.0625, 0.0625, 0.0],        # on the face
                       [0.125, 0.0, 0.0],            # on an edge
                       [0.25, 0.0, 0.0]], np.float32)    # on a vertex
HAND_WANT = np.asarray([0.125, np.hypot(0.125, 0.0625), np.hypot(0.125 * np.sqrt(2), 0.0625),
                        np.hypot(0.125, 0.0625), np.sqrt(2 * 0.125 ** 2 + 0.0625 ** 2),
                        np.sqrt(0.25 ** 2 + 2 * 0.0625 ** 2), np.sqrt(0.25 ** 2 + 2 * 0.0625 ** 2), 0.0, 0.0, 0.0])
# exactly degenerate: two equal vertices (each position), three equal vertices, three collinear vertices (the middle
# one in each position, and unevenly spaced); every product below is exact in fp32, so the normal is exactly zero
_A, _B = [0.125, -0.25, 0.0625], [-0.25, 0.125, 0.3125]
_M, _Q = [-0.0625, -0.0625, 0.1875], [0.03125, -0.15625, 0.125]      # midpoint and quarter point of A B
DEGENERATE = np.asarray([[_A, _A, _B], [_A, _B, _A], [_B, _A, _A], [_A, _A, _A],
                         [_A, _M, _B], [_M, _A, _B], [_A, _B, _M], [_A, _Q, _B], [_Q, _B, _A]], np.float32)


def cases():
    """name -> (points (n,3) fp32, triangles (m,3,3) fp32)"""
    rng = np.random.RandomState(7)
    pts = rng.uniform(-0.5, 0.5, (96, 3)).astype(np.float32)
    return {"random": (pts, random_triangles(300, 1)),
            "wavy 7x9 grid": (pts, grid_triangles(wavy_grid())),
            "sphere with poles": (pts, grid_triangles(sphere_grid())),
            "seven regions": (HAND_PTS, HAND_TRI),
            "degenerate": (np.concatenate([pts[:32], np.asarray([_A, _B, _M], np.float32)]), DEGENERATE)}


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("tmh") / "libtmh.so")
    src = os.path.join(ROOT, "tests", "native", "tri_math_host.cpp")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", out, src], check=True)
    lib = ctypes.CDLL(out)
    lib.tmh_bounds.restype = ctypes.c_int
    lib.tmh_group.restype = ctypes.c_int
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def header_dist2(harness, pts, tri):
    pts, tri = np.ascontiguousarray(pts, np.float32), np.ascontiguousarray(tri, np.float32)
    out = np.full((pts.shape[0], tri.shape[0]), np.nan, np.float32)
    harness.tmh_dist2(_p(pts), pts.shape[0], _p(tri), tri.shape[0], _p(out))
    return out


def measure_bar():
    """4 x E, E the largest difference between the oracle in numpy float32 and in float64 over all cases."""
    E = 0.0
    for name, (pts, tri) in cases().items():
        e = float(np.abs(oracle(pts, tri, np.float32).astype(np.float64) - oracle(pts, tri)).max())
        print("%s: max |oracle fp32 - oracle fp64| = %.3e" % (name, e))
        E = max(E, e)
    print("E = %.3e, bar = %.3e" % (E, 4 * E))
    return 4.0 * E


@pytest.fixture(scope="module")
def bar():
    return measure_bar()


def test_oracle_knows_the_seven_regions():
    assert np.abs(oracle(HAND_PTS, HAND_TRI)[:, 0] - HAND_WANT).max() < 1e-15


def test_header_against_the_float64_oracle(harness, bar):
    """Measured here: E = 1.3e-7 (bar 5.2e-7); the header's largest error over the five cases 1.2e-7."""
    assert 0 < bar < 1e-5
    for name, (pts, tri) in cases().items():
        d2 = header_dist2(harness, pts, tri)
        assert np.isfinite(d2).all() and (d2 >= 0).all(), name
        err = float(np.abs(np.sqrt(d2.astype(np.float64)) - oracle(pts, tri)).max())
        print("%s: %d points x %d triangles, max |header - oracle fp64| = %.3e, bar %.3e"
              % (name, pts.shape[0], tri.shape[0], err, bar))
        assert err <= bar, name
    got = np.sqrt(header_dist2(harness, HAND_PTS, HAND_TRI)[:, 0].astype(np.float64))
    assert np.abs(got - HAND_WANT).max() <= bar
    # a vertex order does not matter (the record is rotated to the vertex opposite the longest edge)
    pts, tri = cases()["random"]
    assert np.abs(np.sqrt(header_dist2(harness, pts, tri[:, [1, 2, 0]]).astype(np.float64)) - oracle(pts, tri)).max() <= bar


def test_degenerate_records_are_finite(harness):
    tri = np.ascontiguousarray(DEGENERATE)
    rec = np.full((tri.shape[0], 16), np.nan, np.float32)
    harness.tmh_records(_p(tri), tri.shape[0], _p(rec))
    assert np.isfinite(rec).all()
    assert (rec[:, 9:12] == 0).all() and (rec[:, 15] == 0).all()      # no normal, no plane term
    assert (rec[3, 3:9] == 0).all() and (rec[3, 12:] == 0).all()      # three equal vertices: a point


def test_bounds_are_certified(harness, bar):
    """For every point and every group of consecutive triangles: lower <= the float64 distance to EVERY triangle of
    the group <= upper (squared), and the lower bound is not trivially zero throughout."""
    group = harness.tmh_group()
    assert group == 8
    useful = 0
    for name, (pts, tri) in cases().items():
        pts, tri = np.ascontiguousarray(pts), np.ascontiguousarray(tri)
        ng = (tri.shape[0] + group - 1) // group
        sph = np.zeros((ng, 4), np.float32)
        lower = np.full((pts.shape[0], ng), np.nan, np.float32)
        upper = np.full((pts.shape[0], ng), np.nan, np.float32)
        assert harness.tmh_bounds(_p(pts), pts.shape[0], _p(tri), tri.shape[0], _p(sph), _p(lower), _p(upper)) == ng
        d = oracle(pts, tri) ** 2
        for g in range(ng):
            block = d[:, g * group:(g + 1) * group]
            assert (lower[:, g].astype(np.float64) <= block.min(1)).all(), (name, g)
            assert (upper[:, g].astype(np.float64) >= block.max(1)).all(), (name, g)
        assert np.isfinite(sph).all() and np.isfinite(upper).all()
        useful += int((lower > 0).sum())
    assert useful > 0


# ---------------------------------------------------------------------------------------------
# exports, header and table
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib_path():
    from parsenet_codebase_amd import build
    return build.build(verbose=False)


def test_library_exports_the_entry_points_at_abi_23(lib_path):
    lib = ctypes.CDLL(lib_path)
    assert all(hasattr(lib, n) for n in NAMES)
    lib.pn_abi_version.restype = ctypes.c_int
    assert lib.pn_abi_version() == 23
    assert lib.pn_trimesh_point_dist_tile() > 0 and lib.pn_trimesh_point_dist_tile() % 64 == 0
    assert lib.pn_trimesh_group() == 8


def test_header_and_ctypes_table_agree(lib_path):
    from parsenet_codebase_amd import _lib
    assert _lib.ABI_VERSION == 23
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NAMES:
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, txt)
        assert m, name
        args = [a for a in m.group(1).split(",") if a.strip() not in ("", "void")]
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(args), name
    assert _lib.SIGNATURES["pn_trimesh_point_dist_f32"][1][8:12] == [ctypes.c_int] * 4


def test_pinned_counters_keep_their_keys():
    from parsenet_codebase_amd import metrics, surface
    assert sorted(metrics.CALLS_PCOVER) == ["fused", "tensor"]
    assert sorted(surface.CALLS_OCCUPANCY) == ["chamfer", "dedicated"]
    assert sorted(surface.CALLS_TRIDIST) == ["distance", "records"]


# ---------------------------------------------------------------------------------------------
# argument checks that need no GPU
# ---------------------------------------------------------------------------------------------
def _surface(kept=True):
    from parsenet_codebase_amd.surface import TrimmedSurface
    g = wavy_grid(4, 5)
    return TrimmedSurface(g.reshape(-1, 3), 4, 5, np.full((3, 4), kept))


def test_a_shape_without_a_kept_triangle_is_a_value_error():
    from parsenet_codebase_amd import metrics, surface
    pts = np.zeros((8, 3), np.float32)
    with pytest.raises(ValueError, match="shape 1 has no kept triangle"):
        surface.point_surface_distance([pts, pts], [[_surface()], [_surface(False), _surface(False)]])
    with pytest.raises(ValueError, match="shape 0 has no kept triangle"):
        surface.point_surface_distance([pts], [[]])
    with pytest.raises(ValueError, match="shape 0 has no kept triangle"):
        metrics.surface_coverage(pts, [_surface(False)])


def test_points_that_are_not_n_by_3_are_a_value_error():
    from parsenet_codebase_amd import metrics, surface
    good = np.zeros((8, 3), np.float32)
    for bad in (np.zeros((8, 2), np.float32), np.zeros((3,), np.float32), np.zeros((0, 3), np.float32),
                np.zeros((2, 4, 3), np.float32)):
        with pytest.raises(ValueError, match=r"shape 1: points must be \(N,3\)"):
            surface.point_surface_distance([good, bad], [[_surface()], [_surface()]])
    with pytest.raises(ValueError, match=r"shape 0: points must be \(N,3\)"):
        metrics.surface_coverage_batch([np.zeros((5, 4), np.float32)], [[_surface()]])
    with pytest.raises(ValueError, match="2 point clouds for 1 lists"):
        surface.point_surface_distance([good, good], [[_surface()]])
