"""CPU-side checks of the cross-cloud neighbour query and the k-NN lifting rules: csrc/knn3_grid_math.h and
csrc/knn_lift_math.h compiled for the host into a serial restatement of the whole query (tests/native/knn3_query_host.cpp:
the reference's grid, the query's clamped cell, rings, the bound, selection by (d, j), padding, interpolation and vote)
against a numpy brute force in the same fp32 arithmetic — exact equality on the adversarial inputs.  This is where the
termination bound is proved for queries OUTSIDE the reference's box: the clamp of kg_cell keeps the cell function
monotone, and the bound's property (no reference point outside ring r with fp32 d < b(r)) is checked directly for such
queries.  Then the library without a GPU: the exports, the launch and workspace functions, every refused argument.
Every comparison is an equality: there is no tolerance in this file."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests.helpers import native
from tests.helpers.native import ROOT
from tests.test_knn3_grid_abi import copies_among_random, lattice, planar

SOURCE = native.source("knn3_query_host.cpp")
QUERY, WORKSPACE, LAUNCHES = "pn_knn3_query_f32", "pn_knn3_query_workspace_bytes", "pn_knn3_query_launches"
INTERPOLATE, VOTE = "pn_knn_interpolate_f32", "pn_knn_vote_i32"
PPCS = (1, 4, 64)      # points per cell: 1 makes many rings, 64 few cells, 4 is the library's own value
KS = (1, 3, 16, 64)


# ---------------------------------------------------------------------------------------------
# the reference definition: brute force in the kernel's fp32 arithmetic
# ---------------------------------------------------------------------------------------------
def brute(R, Q, k, rows=1000):
    """(idx (nq,k) int32, dist (nq,k) fp32) of the queries Q in the reference R: d = ((dx^2 + dy^2) + dz^2) in fp32,
    the k smallest under np.lexsort's order on (j, d), idx -1 / dist +inf from n_r on, dist = (float) sqrt((double) d).
    As tests/test_knn3_grid_gpu.py::brute: np.partition gives every row's k-th smallest d and the lexsort runs over the
    candidates with d <= that value — every tie at the k-th value among them."""
    R, Q = np.ascontiguousarray(R, np.float32).reshape(-1, 3), np.ascontiguousarray(Q, np.float32).reshape(-1, 3)
    nr, nq = R.shape[0], Q.shape[0]
    kk = min(k, nr)
    idx, dd = np.full((nq, k), -1, np.int32), np.full((nq, k), np.inf, np.float32)
    if kk == 0:
        return idx, dd
    with np.errstate(over="ignore", under="ignore"):
        for a in range(0, nq, rows):
            q = Q[a:a + rows]
            dx, dy, dz = q[:, 0, None] - R[None, :, 0], q[:, 1, None] - R[None, :, 1], q[:, 2, None] - R[None, :, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            assert d2.dtype == np.float32
            kth = np.partition(d2, kk - 1, axis=1)[:, kk - 1]
            r, j = np.nonzero(d2 <= kth[:, None])
            d = d2[r, j]
            order = np.lexsort((j, d, r))
            r, j, d = r[order], j[order], d[order]
            first = np.searchsorted(r, np.arange(d2.shape[0]))
            take = first[:, None] + np.arange(kk)[None, :]
            assert (r[take] == np.arange(d2.shape[0])[:, None]).all()
            idx[a:a + rows, :kk] = j[take]
            dd[a:a + rows, :kk] = np.sqrt(d[take].astype(np.float64)).astype(np.float32)
    return idx, dd


def interpolate_ref(values, idx, dist):
    """The interpolation rule in numpy fp64: sequential sums in rank order, then (float).  values (n,C) fp32."""
    nq, k = idx.shape
    C = int(np.prod(values.shape[1:]))
    if values.shape[0] == 0:                                    # no sample: no valid entry in any row
        return np.full((nq, C), np.nan, np.float32)
    values = np.asarray(values, np.float32).reshape(values.shape[0], C)
    num, den = np.zeros((nq, values.shape[1]), np.float64), np.zeros(nq, np.float64)
    with np.errstate(all="ignore"):
        for j in range(k):
            valid = (idx[:, j] >= 0) & (idx[:, j] < values.shape[0])
            w = 1.0 / (dist[:, j].astype(np.float64) + 1e-8)
            t = w[:, None] * values[np.where(valid, idx[:, j], 0)].astype(np.float64)
            num = np.where(valid[:, None], num + t, num)
            den = np.where(valid, den + w, den)
        out = (num / den[:, None]).astype(np.float32)
    valid = (idx >= 0) & (idx < values.shape[0])
    out[np.isnan(dist).any(1) | ~valid.any(1)] = np.nan
    return out


def vote_ref(labels, idx):
    """The vote in plain Python: the most frequent label >= 0 among the valid neighbours, ties to the first in rank."""
    out = np.full(idx.shape[0], -1, np.int32)
    for i, row in enumerate(idx):
        seen = [int(labels[j]) for j in row if 0 <= j < len(labels) and labels[j] >= 0]
        best, most = -1, 0
        for l in seen:                      # in rank order: a later label needs a strictly larger count
            if seen.count(l) > most:
                best, most = l, seen.count(l)
        out[i] = best
    return out


# ---------------------------------------------------------------------------------------------
# inputs (shared with tests/test_knn3_query_gpu.py, which takes them larger)
# ---------------------------------------------------------------------------------------------
def unit_box(n, seed):
    """n uniform points whose bounding box is exactly [0, 1]^3."""
    P = np.random.RandomState(seed).uniform(0, 1, (n, 3)).astype(np.float32)
    P[0], P[1] = 0.0, 1.0
    return P


def outside_queries(per_side, seed, far=50.0):
    """Queries far outside the unit box on each of its six sides, on the eight diagonals, and just outside."""
    rng = np.random.RandomState(seed)
    out = []
    for axis in range(3):
        for sign in (-1.0, 1.0):
            for reach in (far, 0.5, 1e-3):
                q = rng.uniform(0, 1, (per_side, 3))
                q[:, axis] = (1.0 + reach) if sign > 0 else -reach
                out.append(q)
    corners = np.asarray([[sx, sy, sz] for sx in (-far, 1 + far) for sy in (-far, 1 + far) for sz in (-far, 1 + far)])
    out.append(corners)
    out.append(np.repeat(corners, max(per_side // 8, 1), 0) + rng.uniform(-3, 3, (8 * max(per_side // 8, 1), 3)))
    return np.concatenate(out).astype(np.float32)


def face_queries(n, seed, R=8):
    """Queries with coordinates exactly on the faces of the unit box and on interior cell faces (multiples of 1/R)."""
    rng = np.random.RandomState(seed)
    q = rng.uniform(0, 1, (n, 3)).astype(np.float32)
    on = rng.randint(0, R + 1, (n, 3)).astype(np.float32) / np.float32(R)
    pick = rng.uniform(size=(n, 3)) < 0.6
    return np.where(pick, on, q).astype(np.float32)


def corner_crowd(n, seed):
    """A reference crowded into one corner of its box — one far point stretches it — and queries in the empty part."""
    rng = np.random.RandomState(seed)
    P = rng.uniform(0, 0.05, (n, 3)).astype(np.float32)
    P[n // 2] = 1.0
    return P


def adversarial(scale=1):
    """name -> (reference, queries, ks).  scale 1: a few hundred points each (the serial restatement, an n_r n_q brute
    force and three values of ppc); scale 4: the sizes of the GPU tests."""
    rng = np.random.RandomState(40)
    nr, nq = 2048 * (1 if scale == 1 else 4), 60 * scale
    inside = lambda n, s: np.random.RandomState(s).uniform(0, 1, (n, 3)).astype(np.float32)      # noqa: E731
    mixed = np.concatenate([inside(40 * scale, 41), outside_queries(4 * scale, 42)])
    cases = {
        "outside on six sides and diagonally": (unit_box(nr, 43), outside_queries(8 * scale, 44), KS),
        "on box faces and cell faces": (unit_box(nr, 45), face_queries(100 * scale, 46), (1, 16)),
        "reference of one point": (inside(1, 47), mixed, (1, 3)),
        "reference of two points": (inside(2, 48), mixed, (1, 3)),
        "reference of seven points": (inside(7, 49), mixed, (3, 16)),
        "flat reference": (planar(900 * scale), np.concatenate([planar(60 * scale, 50), 2 * mixed - 0.5]), (3, 16)),
        "integer lattice, ties by j": (lattice(10 if scale == 1 else 16, 0.25),
                                        np.concatenate([lattice(6, 0.25), lattice(5, 0.25) + np.float32(0.125),
                                                        lattice(3, 2.0) - np.float32(1.0)]), (3, 16, 64)),
        "coincident reference points": (copies_among_random(600 if scale == 1 else 3000, 400 if scale == 1 else 1000),
                                        np.concatenate([np.asarray([[0.125, -0.25, 0.375]], np.float32),
                                                        rng.uniform(-0.5, 0.5, (50 * scale, 3)).astype(np.float32)]),
                                        (1, 64)),
        "crowded corner, queries in the empty part": (corner_crowd(1500 * scale, 51),
                                                      rng.uniform(0.3, 1.0, (60 * scale, 3)).astype(np.float32), (3, 16)),
        "coordinates near 1e-30": ((unit_box(700, 52) * np.float32(1e-30)).astype(np.float32),
                                   (mixed * np.float32(1e-30)).astype(np.float32), (3,)),
        "coordinates near 1e30": ((unit_box(700, 53) * np.float32(1e30)).astype(np.float32),
                                  (np.clip(mixed, -3, 3) * np.float32(1e30)).astype(np.float32), (3,)),
    }
    for k in KS:
        for n in sorted({0, k - 1, k, k + 1}):
            cases["n_r = %d, k = %d" % (n, k)] = (inside(n, 54 + n), mixed[:40], (k,))
    return cases


# ---------------------------------------------------------------------------------------------
# the host-compiled headers
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    lib = native.build_harness(tmp_path_factory.mktemp("kqh"), "kqh", SOURCE)
    lib.kqh_bound_violations.restype = ctypes.c_longlong
    lib.kqh_interpolate.restype = lib.kqh_vote.restype = None
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def host_query(harness, R, Q, k, ppc):
    """(idx (nq,k) int32, dist (nq,k) fp32, ring (nq) int32) of the serial restatement on one pair of clouds."""
    R, Q = np.ascontiguousarray(R, np.float32).reshape(-1, 3), np.ascontiguousarray(Q, np.float32).reshape(-1, 3)
    nq = Q.shape[0]
    idx, dist, ring = np.full((nq, k), -7, np.int32), np.full((nq, k), -1.0, np.float32), np.full(nq, -7, np.int32)
    assert harness.kqh_query(_p(R), R.shape[0], _p(Q), nq, k, ppc, _p(idx), _p(dist), _p(ring)) == 0
    return idx, dist, ring


def same_bits(a, b):
    """Equal fp32 arrays bit for bit; a NaN equals a NaN (its sign and payload are not part of any contract)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan],
                                                                                      b.view(np.uint32)[~nan])


@pytest.mark.parametrize("name", sorted(adversarial()))
def test_the_restated_query_equals_brute_force(harness, name):
    R, Q, ks = adversarial()[name]
    for k in ks:
        want_idx, want_dist = brute(R, Q, k)
        for ppc in PPCS:
            idx, dist, ring = host_query(harness, R, Q, k, ppc)
            assert np.array_equal(idx, want_idx), (name, k, ppc, int((idx != want_idx).any(1).sum()))
            assert same_bits(dist, want_dist), (name, k, ppc)
            assert (ring >= 0).all() or R.shape[0] == 0


def test_no_reference_point_outside_ring_r_is_nearer_than_the_bound_of_an_outside_query(harness):
    checked = 0
    for name, (R, Q, _) in adversarial().items():
        if R.shape[0] == 0:
            continue
        for ppc in PPCS:
            finite = ctypes.c_longlong()
            bad = harness.kqh_bound_violations(_p(np.ascontiguousarray(R)), R.shape[0], _p(np.ascontiguousarray(Q)),
                                               Q.shape[0], ppc, ctypes.byref(finite))
            assert bad == 0, (name, ppc, bad)
            checked += finite.value
    assert checked > 10000            # positive finite bounds were put to the test, not only 0 and inf


def test_outside_queries_stop_early_and_crowded_corners_run_long(harness):
    """The equality above would also hold for a search that always scans everything.  A query far outside stops at the
    bound of the faces behind it, long before its cube covers the grid; a query in the empty part of a box whose points
    crowd one corner has to run its rings to the crowd."""
    R = unit_box(2048, 43)
    far = np.asarray([[51.0, 0.5, 0.5], [0.5, -50.0, 0.5], [0.5, 0.5, 51.0]], np.float32)
    _, _, ring = host_query(harness, R, far, 3, 4)
    assert (ring < 7).all(), ring                              # 8 cells per axis: covering from a border cell takes 7
    Rc, Qc, _ = adversarial()["crowded corner, queries in the empty part"]
    _, _, ring = host_query(harness, Rc, Qc, 3, 4)
    assert ring.min() >= 1


def test_non_finite_rows(harness):
    R, Q = unit_box(300, 60), unit_box(50, 61)
    for bad in (np.inf, -np.inf, np.nan):
        q = Q.copy()
        q[17, 1] = bad
        idx, dist, _ = host_query(harness, R, q, 5, 4)
        want_idx, want_dist = brute(R, np.delete(q, 17, 0), 5)
        assert (idx[17] == -1).all() and np.isnan(dist[17]).all()
        assert np.array_equal(np.delete(idx, 17, 0), want_idx) and same_bits(np.delete(dist, 17, 0), want_dist)
        r = R.copy()
        r[123, 2] = bad
        idx, dist, _ = host_query(harness, r, Q, 5, 4)
        assert (idx == -1).all() and np.isnan(dist).all()


def test_the_lifting_rules_equal_their_numpy_restatements(harness):
    rng = np.random.RandomState(62)
    R = unit_box(200, 63)
    Q = np.concatenate([R[:20], unit_box(80, 64), outside_queries(1, 65)])       # queries coincident with samples too
    for n, k in ((200, 1), (200, 3), (200, 8), (2, 3), (0, 3)):
        idx, dist, _ = host_query(harness, R[:n], Q, k, 4)
        for C in (1, 3, 50):
            values = rng.normal(0, 10, (n, C)).astype(np.float32)
            out = np.full((Q.shape[0], C), -5.0, np.float32)
            harness.kqh_interpolate(_p(values), n, C, _p(idx), _p(dist), Q.shape[0], k, _p(out))
            assert same_bits(out, interpolate_ref(values, idx, dist)), (n, k, C)
            if n == 0:
                assert np.isnan(out).all()
        labels = rng.randint(-1, 4, n).astype(np.int32)
        out = np.full(Q.shape[0], -5, np.int32)
        harness.kqh_vote(_p(labels), n, _p(idx), Q.shape[0], k, _p(out))
        assert np.array_equal(out, vote_ref(labels, idx)), (n, k)
    # a NaN distance poisons the row; hand-made ties go to the label with the nearer member; labels -1 do not count
    idx = np.asarray([[0, 1, 2, 3], [3, 2, 1, 0], [4, 4, -1, -1], [4, 5, 5, 4], [-1, -1, -1, -1]], np.int32)
    labels = np.asarray([7, 9, 9, 7, -1, 2], np.int32)
    out = np.zeros(5, np.int32)
    harness.kqh_vote(_p(labels), 6, _p(idx), 5, 4, _p(out))
    assert out.tolist() == [7, 7, -1, 2, -1] == vote_ref(labels, idx).tolist()
    dist = np.asarray([[0.0, 1.0, 2.0, np.nan]], np.float32)
    out = np.zeros((1, 1), np.float32)
    harness.kqh_interpolate(_p(np.ones((6, 1), np.float32)), 6, 1, _p(idx[:1].copy()), _p(dist), 1, 4, _p(out))
    assert np.isnan(out).all()


def test_the_sanitized_program_runs_clean_on_the_adversarial_inputs(tmp_path):
    """The restatement as a stand-alone program built with -fsanitize=address,undefined: host code only, not loaded
    into Python.  It must finish without a report, and print brute force's neighbours."""
    exe = str(tmp_path / "knn3_query_host_san")
    subprocess.run(native.GXX + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, SOURCE],
                   check=True)
    for name, (R, Q, ks) in sorted(adversarial().items()):
        k = ks[-1]
        text = "%d %d %d %d\n" % (R.shape[0], Q.shape[0], k, 4) + "".join(
            "%.9g %.9g %.9g\n" % tuple(p) for p in np.concatenate([R.reshape(-1, 3), Q]))
        path = tmp_path / "pair.txt"
        path.write_text(text)
        run = subprocess.run([exe, str(path)], capture_output=True, text=True)
        assert run.returncode == 0 and run.stderr == "", (name, run.returncode, run.stderr[-2000:])
        got = np.asarray([[int(x) for x in line.split()] for line in run.stdout.splitlines()], np.int64)
        want_idx, want_dist = brute(R, Q, k)
        assert np.array_equal(got[:, :k], want_idx), name
        values, labels = R.reshape(-1, 3)[:, :1], (np.arange(R.shape[0]) % 3).astype(np.int32)
        assert same_bits(got[:, k].astype(np.uint32).view(np.float32),
                         interpolate_ref(values, want_idx, want_dist)[:, 0]), name
        assert np.array_equal(got[:, k + 1], vote_ref(labels, want_idx)), name
    assert subprocess.run([exe], input="5 2\n", capture_output=True, text=True).returncode == 2


# ---------------------------------------------------------------------------------------------
# the exports and the argument checks, which run before anything touches a GPU
# ---------------------------------------------------------------------------------------------
def load_raw():
    return native.load_raw((QUERY, WORKSPACE, LAUNCHES, INTERPOLATE, VOTE))


@pytest.fixture(scope="module")
def lib():
    return load_raw()


def test_the_entry_points_are_exported_and_bound(lib):
    from parsenet_codebase_amd import _lib
    v, i, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    assert _lib.SIGNATURES[QUERY] == (i, [v, v, i, v, v, i, i, i, v, v, v, ll, v])
    assert _lib.SIGNATURES[WORKSPACE] == (ll, [ll, ll, i])
    assert _lib.SIGNATURES[LAUNCHES] == (i, [])
    assert _lib.SIGNATURES[INTERPOLATE] == (i, [v, v, i, v, v, v, i, i, i, i, v, v])
    assert _lib.SIGNATURES[VOTE] == (i, [v, v, i, v, v, i, i, i, v, v])
    header = open(os.path.join(ROOT, "include", "parsenet_hip.h")).read()
    for name in (QUERY, WORKSPACE, LAUNCHES, INTERPOLATE, VOTE):
        assert name + "(" in header and hasattr(_lib.load(), name)
    assert lib.pn_abi_version() == 23 == _lib.CONSTANTS["PN_ABI_VERSION"]                   # added symbols only
    assert lib.pn_knn3_query_launches() == 8                                                # a host integer
    # linear in both totals, known from (totalR, totalQ, S) alone
    w = lib.pn_knn3_query_workspace_bytes
    assert w(0, 0, 0) >= 0 and w(-1, 0, 0) == 0 and w(0, -1, 0) == 0 and w(0, 0, -1) == 0
    assert w(2000, 500, 3) - w(1000, 500, 3) == w(3000, 500, 3) - w(2000, 500, 3) == 32 * 1000
    assert w(1000, 2000, 3) - w(1000, 1000, 3) == w(1000, 3000, 3) - w(1000, 2000, 3) == 12 * 1000
    assert w(1000, 500, 3) == 32 * 1000 + 12 * 500 + 44 * 3 + 16
    assert w(3 * 10 ** 8, 3 * 10 ** 8, 1) > 2 ** 32                                         # long long, not int


QUERY_ARGS = ("ref", "off_r", "totalR", "qry", "off_q", "totalQ", "S", "k", "idx", "dist", "ws", "ws_bytes", "stream")


def raw_query(lib, **over):
    """pn_knn3_query_f32 with plausible arguments (never dereferenced by a call that is refused), some replaced."""
    a = dict(ref=64, off_r=64, totalR=10, qry=64, off_q=64, totalQ=20, S=1, k=8, idx=64, dist=None, ws=64,
             ws_bytes=lib.pn_knn3_query_workspace_bytes(10, 20, 1), stream=None)
    a.update(over)
    return lib.pn_knn3_query_f32(*[a[n] for n in QUERY_ARGS])


def test_invalid_arguments_are_refused_before_any_launch(lib):
    """(No GPU is needed to get here: a refused call, and one with nothing to do, launch nothing.)"""
    from parsenet_codebase_amd import _lib
    err = _lib.CONSTANTS["PN_ERR_ARG"]
    need = lib.pn_knn3_query_workspace_bytes(10, 20, 1)
    for over in (dict(k=0), dict(k=65), dict(k=-1), dict(S=-1), dict(totalR=-1), dict(totalQ=-1), dict(ref=None),
                 dict(off_r=None), dict(qry=None), dict(off_q=None), dict(idx=None), dict(ws=None),
                 dict(ws_bytes=need - 1), dict(ws_bytes=0),
                 dict(totalQ=2 ** 31 // 64, k=64, ws_bytes=lib.pn_knn3_query_workspace_bytes(10, 2 ** 31 // 64, 1))):
        assert raw_query(lib, **over) == err, over
        assert b"pn_knn3_query_f32" in lib.pn_last_error()
    assert raw_query(lib, totalQ=0) == 0
    assert raw_query(lib, S=0) == 0
    assert raw_query(lib, totalQ=0, ref=None, qry=None, idx=None, ws=None, ws_bytes=0) == 0
    # the two consumers
    interp = lambda **o: lib.pn_knn_interpolate_f32(*[dict(dict(                               # noqa: E731
        values=64, off_r=64, totalR=10, idx=64, dist=64, off_q=64, totalQ=20, S=1, k=3, C=4, out=64, stream=None), **o)[n]
        for n in ("values", "off_r", "totalR", "idx", "dist", "off_q", "totalQ", "S", "k", "C", "out", "stream")])
    vote = lambda **o: lib.pn_knn_vote_i32(*[dict(dict(                                        # noqa: E731
        labels=64, off_r=64, totalR=10, idx=64, off_q=64, totalQ=20, S=1, k=3, out=64, stream=None), **o)[n]
        for n in ("labels", "off_r", "totalR", "idx", "off_q", "totalQ", "S", "k", "out", "stream")])
    for over in (dict(k=0), dict(k=65), dict(S=-1), dict(totalR=-1), dict(totalQ=-1), dict(off_r=None), dict(idx=None),
                 dict(off_q=None), dict(out=None), dict(totalQ=2 ** 31 // 64, k=64)):
        assert interp(**over) == err and b"pn_knn_interpolate_f32" in lib.pn_last_error(), over
        assert vote(**over) == err and b"pn_knn_vote_i32" in lib.pn_last_error(), over
    for over in (dict(C=0), dict(C=-3), dict(values=None), dict(dist=None), dict(totalQ=2 ** 30, k=1, C=2 ** 9)):
        assert interp(**over) == err, over
    assert vote(labels=None) == err
    assert interp(totalQ=0) == 0 and interp(S=0) == 0 and vote(totalQ=0) == 0 and vote(S=0) == 0


def test_python_argument_checks_need_no_gpu():
    import torch
    from parsenet_codebase_amd import kernels, neighbors
    off = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="MI355X only"):
        kernels.knn3_query(torch.zeros(8, 3), off, torch.zeros(4, 3), off, 3)
    with pytest.raises(RuntimeError, match="MI355X only"):
        neighbors.nearest(torch.zeros(8, 3), torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="MI355X only"):
        neighbors.lift_knn(torch.zeros(4), torch.zeros(8, 3), torch.zeros(4, 3))
    with pytest.raises(ValueError, match="k must be 1 .. 64"):
        neighbors.nearest(torch.zeros(8, 3), torch.zeros(4, 3), k=65)
    with pytest.raises(ValueError, match="k must be 1 .. 64"):
        neighbors.lift_knn(torch.zeros(4), torch.zeros(8, 3), torch.zeros(4, 3), k=0)
