"""CPU-side checks of the uniform-grid neighbour search: csrc/knn3_grid_math.h compiled for the host into a serial
restatement of the whole search (tests/native/knn3_grid_host.cpp: grid, cell function, rings, bound, selection by
(d, j)) against brute force in the same arithmetic (tests.test_point_normals_abi.knn3) — exact equality of the indices
on the adversarial inputs —, the two properties the exactness rests on checked directly (a monotone cell function; no
point outside ring r with fp32 d < b(r)), the non-finite rule, the grid's size, the export of csrc/knn3_grid.hip and its
argument checks."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests.helpers import native
from tests.helpers.native import ROOT
from tests.test_point_normals_abi import knn3

SOURCE = native.source("knn3_grid_host.cpp")
NAME = "pn_knn3_grid_f32"
WORKSPACE = "pn_knn3_grid_workspace_bytes"
PPCS = (1, 4, 64)      # points per cell: 1 makes many rings, 64 few cells, 4 is the library's own value


# ---------------------------------------------------------------------------------------------
# inputs (shared with tests/test_knn3_grid_gpu.py, which takes them larger)
# ---------------------------------------------------------------------------------------------
def tight_pairs(n, seed):
    """The cloud of test_difference_form_neighbours_of_a_ragged_batch: tight pairs at 1e-4 and an exact duplicate."""
    rng = np.random.RandomState(seed)
    p = rng.uniform(-0.5, 0.5, (n, 3)).astype(np.float32)
    p[n // 2:] = p[:n - n // 2] + rng.normal(0, 1e-4, (n - n // 2, 3)).astype(np.float32)
    if n > 5:
        p[5] = p[3]
    return p


def lattice(m, scale=0.25):
    """The m^3 integer lattice scaled by a power of two: points exactly on cell faces, massive ties."""
    g = np.stack(np.meshgrid(np.arange(m), np.arange(m), np.arange(m), indexing="ij"), -1).reshape(-1, 3)
    return (g * scale).astype(np.float32)


def lattice_and_shifted_copy(m, scale=0.25):
    P = lattice(m, scale)
    return np.concatenate([P, P + np.float32(scale / 2)]).astype(np.float32)


def copies_among_random(copies, others, seed=11):
    """``copies`` copies of one point among ``others`` random ones, shuffled."""
    rng = np.random.RandomState(seed)
    P = np.concatenate([np.tile(np.asarray([[0.125, -0.25, 0.375]], np.float32), (copies, 1)),
                        rng.uniform(-0.5, 0.5, (others, 3)).astype(np.float32)])
    return P[rng.permutation(P.shape[0])]


def planar(n, seed=12):
    P = np.random.RandomState(seed).uniform(-1, 1, (n, 3)).astype(np.float32)
    P[:, 2] = np.float32(0.3)
    return P


def collinear(n, seed=13):
    t = np.random.RandomState(seed).uniform(-1, 1, (n, 1))
    return (np.asarray([[0.1, 0.2, -0.3]]) + t * np.asarray([[1.0, -2.0, 0.5]])).astype(np.float32)


def identical(n):
    return np.tile(np.asarray([[0.7, -0.1, 3.0]], np.float32), (n, 1))


def cube_and_far_point(n, seed=14):
    P = np.random.RandomState(seed).uniform(0, 1, (n + 1, 3)).astype(np.float32)
    P[n // 3] = np.float32(1e6)
    return P


def offset_cloud(n, seed=15):
    """A cloud offset by (100, -50, 30) with 1e-4 spacing: the coordinates carry a handful of significant bits."""
    rng = np.random.RandomState(seed)
    return (np.asarray([[100.0, -50.0, 30.0]]) + 1e-4 * rng.uniform(-8, 8, (n, 3))).astype(np.float32)


def adversarial(scale=1):
    """name -> (cloud, ks).  scale 1: a few hundred to 2 000 points (the serial restatement and an n^2 brute force)."""
    return {
        "tight pairs": (tight_pairs(700 * scale, 3), (1, 5, 16, 64)),
        "uniform": (np.random.RandomState(2).uniform(-0.5, 0.5, (2000, 3)).astype(np.float32), (16,)),
        "lattice": (lattice(10 if scale == 1 else 16), (5, 16)),
        "lattice and shifted copy": (lattice_and_shifted_copy(8 if scale == 1 else 16), (16,)),
        "copies among random": (copies_among_random(600 if scale == 1 else 3000, 400 if scale == 1 else 1000), (64,)),
        "planar": (planar(900 * scale), (16,)),
        "collinear": (collinear(500 * scale), (16,)),
        "identical": (identical(300 * scale), (5, 64)),
        "cube and a far point": (cube_and_far_point(1000), (16,)),
        "offset, 1e-4 spacing": (offset_cloud(800 * scale), (16,)),
        "fewer than k": (np.random.RandomState(4).uniform(-1, 1, (7, 3)).astype(np.float32), (16,)),
        "one point": (np.zeros((1, 3), np.float32), (5,)),
    }


# ---------------------------------------------------------------------------------------------
# the host-compiled header
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    lib = native.build_harness(tmp_path_factory.mktemp("kgh"), "kgh", SOURCE)
    lib.kgh_bound_violations.restype = ctypes.c_longlong
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def host_search(harness, P, k, ppc):
    """(idx (n,k) int32, dist (n,k) fp32, ring (n) int32) of the serial restatement on one cloud."""
    P = np.ascontiguousarray(P, np.float32)
    n = P.shape[0]
    idx, dist, ring = np.full((n, k), -7, np.int32), np.full((n, k), -1.0, np.float32), np.full(n, -7, np.int32)
    assert harness.kgh_search(_p(P), n, k, ppc, _p(idx), _p(dist), _p(ring)) == 0
    return idx, dist, ring


def host_cells(harness, P, ppc):
    """(dim (3), cell (n,3), h, number of cells) of the grid of one cloud."""
    P = np.ascontiguousarray(P, np.float32)
    dim, cell, h = np.zeros(3, np.int32), np.zeros((P.shape[0], 3), np.int32), ctypes.c_float()
    cells = harness.kgh_cells(_p(P), P.shape[0], ppc, _p(dim), _p(cell), ctypes.byref(h))
    return dim, cell, h.value, cells


def brute_dist(P, idx):
    """(float) sqrt((double) d) of the neighbours idx, d in knn3's fp32 expression."""
    d = P[:, None, :] - P[idx]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    assert d2.dtype == np.float32
    return np.sqrt(d2.astype(np.float64)).astype(np.float32)


@pytest.mark.parametrize("name", sorted(adversarial()))
def test_the_restated_search_equals_brute_force(harness, name):
    P, ks = adversarial()[name]
    for k in ks:
        want = knn3(P, k)
        for ppc in PPCS:
            idx, dist, ring = host_search(harness, P, k, ppc)
            assert np.array_equal(idx, want), (name, k, ppc, int((idx != want).any(1).sum()))
            assert np.array_equal(dist.view(np.uint32), brute_dist(P, want).view(np.uint32)), (name, k, ppc)
            assert (ring >= 0).all()


def test_the_search_stops_early_on_ordinary_clouds(harness):
    """The equality above would also hold for a search that always scans everything; it does not: on a uniform cloud
    and on a surface most queries stop before their cube covers the grid."""
    P = np.random.RandomState(2).uniform(-0.5, 0.5, (2000, 3)).astype(np.float32)
    for cloud in (P, (P / np.linalg.norm(P, axis=1, keepdims=True)).astype(np.float32)):
        dim, cell, _, _ = host_cells(harness, cloud, 4)
        _, _, ring = host_search(harness, cloud, 8, 4)
        cover = np.maximum(cell, dim - 1 - cell).max(1)
        assert dim.max() >= 5 and (ring < cover).mean() > 0.5, (dim, (ring < cover).mean())


def test_the_cell_function_is_monotone_and_the_grid_is_no_larger_than_the_cloud(harness):
    for name, (P, _) in adversarial().items():
        for ppc in PPCS:
            dim, cell, h, cells = host_cells(harness, P, ppc)
            n = P.shape[0]
            assert cells == int(dim.prod()) and 1 <= cells <= max(1, n // ppc), (name, ppc, dim)
            assert (cell >= 0).all() and (cell < dim).all()
            for a in range(3):
                order = np.argsort(P[:, a], kind="stable")
                assert (np.diff(cell[order, a]) >= 0).all(), (name, ppc, a)
                if np.ptp(P[:, a]) == 0:
                    assert dim[a] == 1, (name, ppc, a)                    # a zero extent: one cell along the axis
    # dense coordinates around every face of a grid: each fp32 number of a stretch, not a sample
    base = np.random.RandomState(1).uniform(0, 1, (4096, 3)).astype(np.float32)
    base[0], base[1] = 0.0, 1.0
    dim, _, h, _ = host_cells(harness, base, 8)
    assert dim.tolist() == [8, 8, 8] and h == 0.125
    for face in range(1, 8):
        start = np.float32(face * h).view(np.uint32) - 200
        xs = (start + np.arange(400, dtype=np.uint32)).view(np.float32)
        probe = base.copy()
        probe[2:402, 0] = xs
        _, cell, _, _ = host_cells(harness, probe, 8)
        got = cell[2:402, 0]
        assert (np.diff(got) >= 0).all() and got[0] == face - 1 and got[-1] == face


def test_no_point_outside_ring_r_is_nearer_than_the_bound(harness):
    checked = 0
    for name, (P, _) in adversarial().items():
        for ppc in PPCS:
            finite = ctypes.c_longlong()
            bad = harness.kgh_bound_violations(_p(np.ascontiguousarray(P)), P.shape[0], ppc, ctypes.byref(finite))
            assert bad == 0, (name, ppc, bad)
            checked += finite.value
    assert checked > 10000            # positive finite bounds were put to the test, not only 0 and inf


def test_the_resolution_is_an_integer_function_of_n(harness):
    for ppc in (1, 8, 64):
        for n in (0, 1, 7, 8, 63, 64, 65, 511, 512, 999, 1000, 1001, 10 ** 6, 2 ** 31 - 1):
            R = harness.kgh_resolution(n, ppc)
            assert R >= 1 and (R == 1 or ppc * R ** 3 <= n) and ppc * (R + 1) ** 3 > n, (n, ppc, R)
    assert 1 <= harness.kgh_default_ppc() <= 64


def test_a_non_finite_coordinate_gives_self_rows_and_nan_distances(harness):
    for bad in (np.inf, -np.inf, np.nan):
        P = np.random.RandomState(6).uniform(-1, 1, (300, 3)).astype(np.float32)
        P[123, 1] = bad
        idx, dist, _ = host_search(harness, P, 9, 8)
        assert np.array_equal(idx, np.repeat(np.arange(300, dtype=np.int32)[:, None], 9, 1))
        assert np.isnan(dist).all()
    # the largest finite coordinates overflow the extent and the distances, and still give brute force's neighbours
    P = np.random.RandomState(7).uniform(-1, 1, (200, 3)).astype(np.float32)
    P[:3] = np.asarray([[3e38, 0, 0], [-3e38, 0, 0], [0, 3e38, 1]], np.float32)
    with np.errstate(over="ignore"):
        want = knn3(P, 6)
    assert np.array_equal(host_search(harness, P, 6, 1)[0], want)


def test_the_program_reads_a_cloud_from_stdin_and_a_file(harness, tmp_path):
    exe = native.build_program(tmp_path, "knn3_grid_host", SOURCE)
    P, k = tight_pairs(150, 1), 7
    text = "%d %d %d\n" % (P.shape[0], k, 2) + "".join("%.9g %.9g %.9g\n" % tuple(p) for p in P)
    path = tmp_path / "cloud.txt"
    path.write_text(text)
    for run in (subprocess.run([exe], input=text, capture_output=True, text=True, check=True),
                subprocess.run([exe, str(path)], capture_output=True, text=True, check=True)):
        got = np.asarray([[int(x) for x in line.split()] for line in run.stdout.splitlines()], np.int32)
        assert np.array_equal(got, knn3(P, k))
    assert subprocess.run([exe], input="5 2\n", capture_output=True, text=True).returncode == 2


# ---------------------------------------------------------------------------------------------
# the export and the argument checks, which run before anything touches a GPU
# ---------------------------------------------------------------------------------------------
def load_raw():
    return native.load_raw((NAME, WORKSPACE))


@pytest.fixture(scope="module")
def lib():
    return load_raw()


def test_the_entry_points_are_exported_and_bound(lib):
    from parsenet_codebase_amd import _lib
    v, i, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    assert _lib.SIGNATURES[NAME] == (i, [v, v, i, i, i, i, v, v, v, ll, v])
    assert _lib.SIGNATURES[WORKSPACE] == (ll, [ll, i])
    header = open(os.path.join(ROOT, "include", "parsenet_hip.h")).read()
    assert NAME + "(" in header and WORKSPACE + "(" in header
    assert lib.pn_abi_version() == 23 == _lib.CONSTANTS["PN_ABI_VERSION"]                   # added symbols only
    assert hasattr(_lib.load(), NAME) and hasattr(_lib.load(), WORKSPACE)
    # linear in total, known from (total, S) alone
    w = lib.pn_knn3_grid_workspace_bytes
    assert w(0, 0) >= 0 and w(1000, 3) > 28 * 1000
    assert w(2000, 3) - w(1000, 3) == w(3000, 3) - w(2000, 3) <= 64 * 1000
    assert w(3 * 10 ** 8, 1) > 2 ** 32                                                      # long long, not int


ARGS = ("pts", "off", "S", "total", "max_n", "k", "idx", "dist", "ws", "ws_bytes", "stream")


def raw_call(lib, **over):
    """pn_knn3_grid_f32 with plausible arguments (never dereferenced by a call that is refused), some replaced."""
    a = dict(pts=64, off=64, S=1, total=10, max_n=10, k=8, idx=64, dist=None, ws=64,
             ws_bytes=lib.pn_knn3_grid_workspace_bytes(10, 1), stream=None)
    a.update(over)
    return lib.pn_knn3_grid_f32(*[a[n] for n in ARGS])


def check_invalid_arguments(lib, **real):
    """k out of range, S < 0, a null required pointer, a short workspace: PN_ERR_ARG; nothing to do: 0."""
    from parsenet_codebase_amd import _lib
    err = _lib.CONSTANTS["PN_ERR_ARG"]
    need = lib.pn_knn3_grid_workspace_bytes(real.get("total", 10), real.get("S", 1))
    for over in (dict(k=0), dict(k=65), dict(k=-1), dict(S=-1), dict(total=-1), dict(pts=None), dict(off=None),
                 dict(idx=None), dict(ws=None), dict(ws_bytes=need - 1), dict(ws_bytes=0)):
        assert raw_call(lib, **dict(real, **over)) == err, over
        assert b"pn_knn3_grid_f32" in lib.pn_last_error()
    assert raw_call(lib, **dict(real, total=0)) == 0
    assert raw_call(lib, **dict(real, S=0)) == 0
    assert raw_call(lib, **dict(real, total=0, pts=None, idx=None, ws=None, ws_bytes=0)) == 0


def test_invalid_arguments_are_refused_before_any_launch(lib):
    """(No GPU is needed to get here: a refused call, and one with nothing to do, launch nothing.)"""
    check_invalid_arguments(lib)


def test_python_argument_checks_need_no_gpu():
    import torch
    from parsenet_codebase_amd import kernels, point_normals
    with pytest.raises(RuntimeError, match="MI355X only"):
        kernels.knn3_grid(torch.zeros(8, 3), torch.zeros(2, dtype=torch.int32), 8, 3)
    with pytest.raises(RuntimeError, match="MI355X only"):
        point_normals.estimate_normals(torch.zeros(8, 3), search="grid")
    with pytest.raises(RuntimeError, match="MI355X only"):
        point_normals.orient_normals(torch.zeros(8, 3), torch.zeros(8, 3), search="auto")
