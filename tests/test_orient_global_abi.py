"""CPU-side checks of the global-memory orientation engine (csrc/orient_global.hip, steps and schedule
csrc/orient_global_math.h): the three exports, their signatures and argument checks, the workspace and the schedule;
the Python argument checks; and the host simulation (tests/native/orient_global_host.cpp), which runs the launches of
the schedule serially on the kernels' own step source and must equal the Kruskal restatement
(tests/native/orient_math_host.cpp) in every bit of normals, flip and seed, within the schedule and with no cap hit —
on every input of tests/test_orient_normals_abi.py, on the chain adversary (round one hooks the whole cloud into one
chain, so that more than one compress pass is needed) and on two closed shapes of 12 000 and 20 000 points."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests.helpers import native
from tests.helpers.native import ROOT
from tests.test_orient_normals_abi import (UP, build_harness, canonical_normals, closed_shapes, host_orient, lattice,
                                           py_weights, same_bits, torus)
from tests.test_point_normals_abi import knn3, sphere

SOURCE = native.source("orient_global_host.cpp")
STEPS = os.path.join(ROOT, "parsenet_codebase_amd", "csrc", "orient_global_math.h")
NAME = "pn_orient_normals_global_f32"
ARGS = ("pts", "off", "S", "total", "max_n", "idx", "k", "normals_in", "normals_out", "flip", "seed", "ws", "ws_bytes",
        "stream")


def constant(name):
    """A ``#define NAME integer`` of the step header."""
    return int(re.search(r"^#define %s (\d+)\b" % name, open(STEPS).read(), flags=re.M).group(1))


BLOCK, MAX_BLOCKS, WALK = constant("OG_BLOCK"), constant("OG_MAX_BLOCKS"), constant("OG_WALK")
STRIDE = BLOCK * MAX_BLOCKS


# ---------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------
def chain(n=5000):
    """The chain adversary: n points on a line and, at k = 3, normals (cos t_i, sin t_i, 0) whose angle steps fall
    linearly from 0.5 to 0.05 rad.  Returns (points, idx, normals)."""
    P = np.stack([np.arange(n) / 64.0, np.zeros(n), np.zeros(n)], 1).astype(np.float32)
    t = np.concatenate([[0.0], np.cumsum(np.linspace(0.5, 0.05, n - 1))])
    nrm = np.stack([np.cos(t), np.sin(t), np.zeros(n)], 1).astype(np.float32)
    i = np.arange(n)
    idx = np.stack([i, np.clip(i - 1, 0, None), np.clip(i + 1, None, n - 1)], 1)
    idx[0], idx[-1] = (0, 1, 2), (n - 1, n - 2, n - 3)
    return P, np.ascontiguousarray(idx, np.int32), nrm


def check_chain_precondition(idx, nrm):
    """The weights fall strictly along the line and the smallest entry at every vertex leads to its successor (at the
    last vertex: back to its predecessor, a mutual pick), so round one hooks one chain of length n - 1."""
    n = idx.shape[0]
    w, _, valid = py_weights(nrm, idx)
    assert valid[:, 1:].all() and n > WALK * WALK and n >= 5000
    step = w[np.arange(1, n), 1]                                        # entry i -> i - 1, i = 1 .. n - 1
    assert (idx[1:, 1] == np.arange(n - 1)).all() and (np.diff(step.astype(np.float64)) < 0).all()
    smallest = np.full(n, np.inf)
    partner = np.full(n, -1)
    for i, s in zip(*np.nonzero(valid)):
        for a, b in ((i, idx[i, s]), (idx[i, s], i)):
            if w[i, s] < smallest[a]:
                smallest[a], partner[a] = w[i, s], b
    assert (partner[:-1] == np.arange(1, n)).all() and partner[-1] == n - 2


def knn_blocks(P, k, rows=256):
    """(n,k) int32 neighbours of a large cloud, fp32 distances as knn3 forms them, computed in blocks of rows; nearest
    first, equal distances to the smaller index (a tie AT the k-th distance may keep either point, which no check
    here depends on: every comparison runs both sides on the same lists)."""
    P = np.asarray(P, np.float32)
    out = np.empty((P.shape[0], k), np.int32)
    for a in range(0, P.shape[0], rows):
        d = P[a:a + rows, None, :] - P[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        near = np.sort(np.argpartition(d2, k - 1, axis=1)[:, :k], axis=1)
        order = np.argsort(np.take_along_axis(d2, near, 1), axis=1, kind="stable")
        out[a:a + rows] = np.take_along_axis(near, order, 1)
    return out


def big_sphere(n=12000, seed=7):
    """The jittered sphere of tests/test_orient_normals_gpu.py's limit test, scaled up."""
    outward = sphere(n).astype(np.float64)
    return (outward * (1.0 + 0.002 * np.random.RandomState(seed).standard_normal((n, 1)))).astype(np.float32), outward


def big_torus():
    return torus(nu=200, nv=100)


# ---------------------------------------------------------------------------------------------
# the host simulation
# ---------------------------------------------------------------------------------------------
def build_simulation(directory):
    return native.build_harness(directory, "ogh", SOURCE)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory.mktemp("omh_global"))


@pytest.fixture(scope="module")
def simulation(tmp_path_factory):
    return build_simulation(tmp_path_factory.mktemp("ogh"))


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def simulate(simulation, P, off, idx, normals, order=0):
    """((normals, flip, seed), report) of the serial simulation over a ragged batch."""
    P, normals = np.ascontiguousarray(P, np.float32), np.ascontiguousarray(normals, np.float32)
    off, idx = np.ascontiguousarray(off, np.int32), np.ascontiguousarray(idx, np.int32)
    total, k = idx.shape
    out = np.full((total, 3), np.nan, np.float32)
    flip, seed = np.full(total, -7, np.int32), np.full(total, -7, np.int32)
    report = np.full(7, -1, np.int32)
    simulation.ogh_orient(_p(P), _p(off), off.shape[0] - 1, _p(idx), k, _p(normals), order, _p(out), _p(flip), _p(seed),
                          _p(report))
    names = ("sufficed", "rounds", "rounds_scheduled", "passes", "passes_scheduled", "launches", "depth")
    return (out, flip, seed), dict(zip(names, report.tolist()))


def agree(harness, simulation, P, idx, normals, off=None):
    """The simulation, visiting the elements of a launch in either order, against Kruskal: every bit, and the schedule
    sufficed.  Returns (Kruskal's result, the report of the ascending order)."""
    off = [0, np.asarray(P).shape[0]] if off is None else off
    want = host_orient(harness, P, off, idx, normals)
    for order in (1, 0):
        got, report = simulate(simulation, P, off, idx, normals, order)
        assert same_bits(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), order
        assert report["sufficed"] == 1, report
        assert report["rounds"] < report["rounds_scheduled"] and report["passes"] <= report["passes_scheduled"], report
    return want, report


def test_the_schedule_is_the_one_the_library_reports(simulation, lib):
    assert [simulation.ogh_constant(i) for i in range(4)] == [BLOCK, MAX_BLOCKS, STRIDE, WALK]
    last = 0
    for n in list(range(0, 70)) + [WALK ** 2 - 1, WALK ** 2, WALK ** 2 + 1, 10240, 10241, 10 ** 5, 10 ** 6, 2 ** 31 - 1]:
        rounds, passes = simulation.ogh_rounds(n), simulation.ogh_passes(n)
        assert rounds == max(int(np.ceil(np.log2(max(n, 1)))), 0) + 1 and WALK ** passes >= n
        assert passes == 1 or WALK ** (passes - 1) < n
        assert rounds <= simulation.ogh_constant(4) and passes < simulation.ogh_constant(5)
        launches = lib.pn_orient_normals_global_launches(n)
        assert launches == simulation.ogh_launches(n) == 1 + rounds * (2 + passes) + 2
        assert launches >= last                                          # monotone in max_n
        last = launches
    assert lib.pn_orient_normals_global_launches(-5) == lib.pn_orient_normals_global_launches(0)
    assert last < 300                                                    # O(log n) rounds of a few launches


def test_simulation_on_every_input_of_the_one_workgroup_tests(harness, simulation):
    for k in (8, 16):
        for name, (P, outward) in closed_shapes().items():
            idx = knn3(P, k)
            (got, _, seed), report = agree(harness, simulation, P, idx, canonical_normals(P, idx))
            assert ((got.astype(np.float64) * outward).sum(1) > 0).all(), (name, k)
            print("%s, k = %d: %s" % (name, k, report))
    # the all-ties lattice, whole and half negated
    P = lattice()
    n = P.shape[0]
    for k in (5, 16):
        idx = knn3(P, k)
        agree(harness, simulation, P, idx, np.tile(UP, (n, 1)))
        down = np.random.RandomState(k).permutation(n) < n // 2
        for mask in (down, ~down):
            (got, flip, seed), _ = agree(harness, simulation, P, idx, np.where(mask[:, None], -UP, UP))
            assert np.array_equal(got, np.tile(UP, (n, 1))) and np.array_equal(flip == 1, mask) and not seed.any()
    # duplicated points
    base, _ = torus(nu=12, nv=8)
    P = np.concatenate([base, base])[np.random.RandomState(1).permutation(2 * base.shape[0])]
    for k in (3, 8):
        agree(harness, simulation, P, knn3(P, k), canonical_normals(P, knn3(P, 12)))
    # tiny clouds and padding
    one = np.asarray([[0.5, 0.25, -1.0]], np.float32)
    for nz in (1.0, -1.0):
        agree(harness, simulation, one, knn3(one, 4), np.asarray([[0, 0, nz]], np.float32))
    two = np.asarray([[0, 0, 0], [0.5, 0, 0.25]], np.float32)
    agree(harness, simulation, two, knn3(two, 5), np.asarray([[0, 0.6, 0.8], [0, -0.6, -0.8]], np.float32))
    P = lattice(3, 3)
    (_, flip, seed), _ = agree(harness, simulation, P, knn3(P, 1), np.tile(-UP, (9, 1)))
    assert flip.all() and seed.tolist() == list(range(9))               # k = 1: no entry at all
    P = sphere(7)
    nrm = canonical_normals(P, knn3(P, 7))
    for k in (8, 16, 64):
        agree(harness, simulation, P, knn3(P, k), nrm)
    wild = knn3(P, 4)
    wild[:, 3] = np.where(np.arange(7) % 2 == 0, -1, 7)                 # outside the segment: dropped
    agree(harness, simulation, P, wild, nrm)
    # zero normals and a level seed
    P = sphere(50)
    idx = knn3(P, 6)
    agree(harness, simulation, P, idx, np.zeros((50, 3), np.float32))
    nrm = canonical_normals(P, idx)
    nrm[20] = 0
    agree(harness, simulation, P, idx, nrm)
    P = lattice(4, 4)
    P[5, 2] = 0.5
    idx = knn3(P, 5)
    for nz in (0.0, -0.0):
        for nx in (1.0, -1.0):
            agree(harness, simulation, P, idx, np.tile(np.asarray([nx, 0, nz], np.float32), (16, 1)))
    nrm = np.tile(-UP, (16, 1))
    nrm[5] = 0
    agree(harness, simulation, P, idx, nrm)
    # a ragged batch with empty segments: the schedule of the largest segment serves every segment
    clouds = [sphere(64), np.zeros((0, 3), np.float32), sphere(1), sphere(130), sphere(63)]
    off = np.concatenate([[0], np.cumsum([c.shape[0] for c in clouds])])
    idx = np.concatenate([knn3(c, 5) if c.shape[0] else np.zeros((0, 5), np.int32) for c in clouds])
    nrm = np.random.RandomState(3).standard_normal((off[-1], 3)).astype(np.float32)
    agree(harness, simulation, np.concatenate(clouds), idx, nrm, off)


def test_the_chain_adversary_needs_more_than_one_compress_pass(harness, simulation):
    P, idx, nrm = chain()
    n = P.shape[0]
    check_chain_precondition(idx, nrm)
    _, report = agree(harness, simulation, P, idx, nrm)
    print(report)
    assert report["depth"] == n - 2                   # round one: 0 -> 1 -> ... -> n - 2 <- n - 1, one chain over all n
    assert report["rounds"] == 1 and 2 <= report["passes"] <= report["passes_scheduled"] == 3


@pytest.fixture(scope="module")
def large_shapes():
    """{name: (points, outward normals, idx at k = 16, canonical-sign normals)}, computed once."""
    out = {}
    for name, (P, outward) in (("sphere 12000", big_sphere()), ("torus 200 x 100", big_torus())):
        idx = knn_blocks(P, 16)
        out[name] = (P, outward, idx, canonical_normals(P, idx))
    return out


def test_large_closed_shapes(harness, simulation, large_shapes):
    """The quality condition goes on the oracle, at k = 16 on both shapes: after orientation every normal has a positive
    dot with the analytic outward normal.  The simulation then has to equal the oracle in every bit."""
    for name, (P, outward, idx, nrm) in large_shapes.items():
        assert P.shape[0] > 10240
        before = float(((nrm.astype(np.float64) * outward).sum(1) > 0).mean())
        (got, flip, seed), report = agree(harness, simulation, P, idx, nrm)
        after = (got.astype(np.float64) * outward).sum(1) > 0
        print("%s: outward before %.3f, after %.3f; %s" % (name, before, after.mean(), report))
        assert 0.3 < before < 0.7 and after.all() and np.unique(seed).size == 1, name


def test_the_program_reads_a_cloud_and_reports(tmp_path):
    exe = native.build_program(tmp_path, "orient_global_host", SOURCE)
    oracle = native.build_program(tmp_path, "orient_math_host", native.source("orient_math_host.cpp"))
    P, _ = torus(nu=16, nv=9)
    k = 6
    idx = knn3(P, k)
    nrm = canonical_normals(P, idx)
    text = "%d %d\n" % (P.shape[0], k) + "".join("%.9g %.9g %.9g %.9g %.9g %.9g\n" % (tuple(p) + tuple(n))
                                                  for p, n in zip(P, nrm))
    text += "".join(" ".join(str(j) for j in row) + "\n" for row in idx)
    path = tmp_path / "torus.txt"
    path.write_text(text)
    want = subprocess.run([oracle], input=text, capture_output=True, text=True, check=True).stdout
    for run in (subprocess.run([exe], input=text, capture_output=True, text=True, check=True),
                subprocess.run([exe, str(path)], capture_output=True, text=True, check=True)):
        assert run.stdout == want and run.stderr.startswith("sufficed 1, rounds ")
    assert subprocess.run([exe], input="5 0\n", capture_output=True, text=True).returncode == 2
    assert subprocess.run([exe], input="2 2\n0 0 0 0 0 1\n", capture_output=True, text=True).returncode == 2


# ---------------------------------------------------------------------------------------------
# the exports and the argument checks, which run before anything touches a GPU
# ---------------------------------------------------------------------------------------------
def load_raw():
    return native.load_raw((NAME, "pn_orient_normals_global_workspace_bytes", "pn_orient_normals_global_launches",
                            "pn_orient_normals_max_points"))


@pytest.fixture(scope="module")
def lib():
    return load_raw()


def test_the_entry_points_are_exported_and_bound(lib):
    from parsenet_codebase_amd import _lib
    v, i, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    assert _lib.SIGNATURES[NAME] == (i, [v, v, i, i, i, v, i, v, v, v, v, v, ll, v])
    assert _lib.SIGNATURES["pn_orient_normals_global_workspace_bytes"] == (ll, [ll, i])
    assert _lib.SIGNATURES["pn_orient_normals_global_launches"] == (i, [i])
    assert lib.pn_abi_version() == 23 == _lib.CONSTANTS["PN_ABI_VERSION"]                   # added symbols only
    assert lib.pn_orient_normals_max_points() == 10240
    header = open(os.path.join(ROOT, "include", "parsenet_hip.h")).read()
    assert all(name + "(" in header for name in (NAME, "pn_orient_normals_global_workspace_bytes",
                                                 "pn_orient_normals_global_launches"))


def test_the_workspace_is_linear_in_total(lib):
    ws = lib.pn_orient_normals_global_workspace_bytes
    base = ws(0, 1)
    assert 0 < base <= 4096
    per_point = ws(1, 1) - base
    assert 12 <= per_point <= 32                                        # a word and a 64-bit slot at the least
    for total in (2, 1000, 10241, 10 ** 6, 2 ** 31 - 1):
        for S in (1, 7):
            assert ws(total, S) == base + per_point * total
    assert ws(-1, 1) == 0 and ws(5, -1) == 0


def raw_call(lib, **over):
    """pn_orient_normals_global_f32 with plausible arguments (never dereferenced by a refused call), some replaced."""
    a = dict(pts=64, off=64, S=1, total=10, max_n=10, idx=64, k=8, normals_in=64, normals_out=128, flip=None, seed=None,
             ws=256, ws_bytes=None, stream=None)
    a.update(over)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = lib.pn_orient_normals_global_workspace_bytes(max(a["total"], 0), max(a["S"], 0))
    return lib.pn_orient_normals_global_f32(*[a[n] for n in ARGS])


def check_invalid_arguments(lib, **real):
    """The checks of pn_orient_normals_f32, and max_n < 0, a NULL or short workspace, total * k >= 2^31: PN_ERR_ARG;
    nothing to do: 0."""
    from parsenet_codebase_amd import _lib
    err = _lib.CONSTANTS["PN_ERR_ARG"]
    total = real.get("total", 10)
    need = lib.pn_orient_normals_global_workspace_bytes(total, 1)
    alias = dict(normals_out=real.get("normals_in", 64))
    for over in (dict(k=0), dict(k=65), dict(k=-3), dict(S=-1), dict(total=-1), dict(pts=None), dict(off=None),
                 dict(idx=None), dict(normals_in=None), dict(normals_out=None), alias, dict(max_n=-1), dict(ws=None),
                 dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(ws_bytes=-1),
                 dict(total=2 ** 26, k=32, ws_bytes=2 ** 40), dict(total=2 ** 31 - 1, k=2, ws_bytes=2 ** 40)):
        assert raw_call(lib, **dict(real, **over)) == err, over
        assert NAME.encode() in lib.pn_last_error()
    assert raw_call(lib, **dict(real, total=0)) == 0
    assert raw_call(lib, **dict(real, S=0)) == 0
    assert raw_call(lib, **dict(real, total=0, pts=None, idx=None, normals_in=None, normals_out=None, ws=None,
                                ws_bytes=0)) == 0


def test_invalid_arguments_are_refused_before_any_launch(lib):
    """(No GPU is needed to get here: a refused call, and one with nothing to do, launch nothing.)"""
    check_invalid_arguments(lib)


def test_python_argument_checks_need_no_gpu():
    import torch
    from parsenet_codebase_amd import kernels, point_normals
    z = torch.zeros(8, 3)
    for bad in ("lds", "Global", True, 0):
        with pytest.raises(ValueError, match="engine must be"):
            point_normals.orient_normals(z, z, engine=bad)
        with pytest.raises(ValueError, match="engine must be"):
            point_normals.estimate_normals(z, orient="mst", engine=bad)
    for engine in ("global", "auto"):
        with pytest.raises(ValueError, match="engine=.* without orient"):
            point_normals.estimate_normals(z, engine=engine)
        with pytest.raises(RuntimeError, match="MI355X only"):
            point_normals.orient_normals(z, z, engine=engine)
        with pytest.raises(RuntimeError, match="MI355X only"):
            point_normals.estimate_normals(z, orient="mst", engine=engine)
    with pytest.raises(ValueError, match="viewpoint"):
        point_normals.estimate_normals(z, orient="mst", viewpoint=torch.zeros(3), engine="global")
    with pytest.raises(RuntimeError, match="MI355X only"):
        kernels.orient_normals_global(z, [0, 8], torch.zeros(8, 3, dtype=torch.int32), 3, z)
