"""CPU-side checks of the Euclidean cluster extraction: csrc/cluster_math.h compiled for the host into a serial
simulation of the kernels' schedule (tests/native/cluster_host.cpp: bounds, cells, scan, scatter, the Boruvka rounds of
ball searches, hooks and compress passes, sizes, numbers, labels) against ``cluster_numpy``, an independent numpy
restatement of the definition (the fp32 distance matrix with the same parenthesisation, a union of the index sets that
``np.nonzero(d <= r2)`` joins, numbering by first index) — every output exactly equal, with both orders of arrival —,
the exact properties of the definition, the stand-alone program under the address and undefined-behaviour sanitizers,
the export of csrc/cluster.hip, its schedule, its workspace and its argument checks."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests.helpers import native
from tests.test_fps_abi import same
from tests.test_knn3_grid_abi import collinear, copies_among_random, lattice, offset_cloud, planar

SOURCE = native.source("cluster_host.cpp")
NAMES = ("pn_cluster_f32", "pn_cluster_workspace_bytes", "pn_cluster_launches")
BLOCK = 1024     # rows of the distance matrix formed at a time


# ---------------------------------------------------------------------------------------------
# the definition, in numpy (shared with tests/test_cluster_gpu.py)
# ---------------------------------------------------------------------------------------------
def radius_status(r):
    """0, or -2 where the fp32 radius or its fp32 square is no positive finite number."""
    r = np.float32(r)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        r2 = np.float32(r * r)
    return 0 if (r > 0 and np.isfinite(r) and r2 > 0 and np.isfinite(r2)) else -2


STRIP = 32       # ... and the rows worked on at once, so that the arithmetic stays in the cache


def true_positions(mask):
    """np.flatnonzero of a sparse C-contiguous bool array, eight entries at a time: the words that hold a True first."""
    flat = mask.reshape(-1)
    whole = flat.size // 8 * 8
    words = np.flatnonzero(flat[:whole].view(np.uint64))
    cand = (words[:, None] * 8 + np.arange(8)[None, :]).reshape(-1)
    return np.concatenate([cand[flat[cand]], whole + np.flatnonzero(flat[whole:])])


def components_numpy(P, r):
    """comp (n) int64: the lowest index of the connected component of every point.  The fp32 distances of BLOCK rows
    against all, ((dx dx + dy dy) + dz dz) rounded once per operation, give the neighbour list of every row; a
    union-find (the root of a set is its lowest index, every root found is linked to the lowest one) joins them."""
    n = P.shape[0]
    with np.errstate(over="ignore", under="ignore"):
        r2 = np.float32(np.float32(r) * np.float32(r))
    up = np.arange(n)
    D, T = np.empty((2, min(STRIP, n), n), np.float32)                     # (two buffers, reused by every strip)
    x, y, z = (np.ascontiguousarray(P[:, a]) for a in range(3))
    for b in range(0, n, BLOCK):
        lists = []                                                         # the neighbours of the rows of this block
        for s in range(b, min(b + BLOCK, n), STRIP):
            Q = P[s:s + STRIP]
            d, t = D[:Q.shape[0]], T[:Q.shape[0]]
            with np.errstate(over="ignore", under="ignore", invalid="ignore"):
                np.subtract(Q[:, None, 0], x[None, :], out=d)
                np.multiply(d, d, out=d)
                np.subtract(Q[:, None, 1], y[None, :], out=t)
                np.multiply(t, t, out=t)
                np.add(d, t, out=d)
                np.subtract(Q[:, None, 2], z[None, :], out=t)
                np.multiply(t, t, out=t)
                np.add(d, t, out=d)
            assert d.dtype == np.float32
            rows, cols = np.divmod(true_positions(d <= r2), n)
            lists.extend(np.split(cols, np.searchsorted(rows, np.arange(1, Q.shape[0]))))
        for near in lists:                                                 # (the point itself is among them: d = 0)
            if near.size < 2:
                continue
            roots = up[near]
            while True:                                                    # find, all neighbours at once
                above = up[roots]
                if np.array_equal(above, roots):
                    break
                roots = above
            low = roots.min()
            up[roots] = low                                                # union: every root under the lowest one
            up[near] = low                                                 # ... and the paths shortened
    while True:
        above = up[up]
        if np.array_equal(above, up):
            return up
        up = above


def cluster_numpy(P, r, min_size=1):
    """One cloud by the definition: (label (n) int32, ncomp int, count, first (n) int32, ndrop int); the component
    arrays in the first ncomp rows, -1 behind them; ncomp -1 / -2: the statuses."""
    P = np.ascontiguousarray(P, np.float32).reshape(-1, 3)
    n = P.shape[0]
    label, count, first = (np.full(n, -1, np.int32) for _ in range(3))
    status = -1 if not np.isfinite(P).all() else radius_status(r)
    if status or n == 0:
        return label, status, count, first, n
    comp = components_numpy(P, r)
    heads, sizes = np.unique(comp, return_counts=True)                     # ascending lowest index
    assert np.array_equal(comp[heads], heads)
    kept = sizes >= min_size
    C = int(kept.sum())
    number = np.full(n, -1, np.int32)
    number[heads[kept]] = np.arange(C)
    label = number[comp]
    count[:C], first[:C] = sizes[kept], heads[kept]
    return label, C, count, first, int((label < 0).sum())


def cluster_numpy_batch(clouds, radii, min_size=1):
    """A ragged batch: (label (total), ncomp (S), count, first (total), ndrop (S))."""
    out = [cluster_numpy(P, r, min_size) for P, r in zip(clouds, radii)]
    return tuple(np.asarray([o[t] for o in out], np.int32) if t in (1, 4) else np.concatenate([o[t] for o in out])
                 for t in range(5))


def check_properties(P, result):
    """The exact properties of one valid cloud."""
    label, C, count, first, ndrop = result
    n = P.shape[0]
    assert C >= 0 and (count[C:] == -1).all() and (first[C:] == -1).all() and (count[:C] >= 1).all()
    assert (np.diff(first[:C]) > 0).all()                                   # first ascends
    assert np.array_equal(label[first[:C]], np.arange(C))
    assert np.array_equal(np.bincount(label[label >= 0], minlength=C), count[:C])
    assert ndrop + count[:C].sum() == n and ndrop == (label == -1).sum() and label.min(initial=0) >= -1
    for c in range(C):                                                      # first is the lowest index of the component
        assert np.flatnonzero(label == c)[0] == first[c]


def partition(P, label):
    """The partition as a set of frozen sets of point coordinates' row bytes with multiplicity (index-free)."""
    groups = {}
    for i, c in enumerate(label.tolist()):
        groups.setdefault(c, []).append(P[i].tobytes())
    return sorted(sorted(g) for g in groups.values())


def uniform(n, seed=None):
    return np.random.RandomState(n if seed is None else seed).uniform(-1, 1, (n, 3)).astype(np.float32)


def between(n):
    """A radius at which uniform(n) falls into many components of mixed sizes (mean degree about 1.4)."""
    return 1.4 / max(n, 2) ** (1.0 / 3.0)


ALONE, ONE = 1e-5, 4.0             # on uniform(-1, 1): every point alone; above the extent: one component, one cell
SIZES = (1, 2, 3, 65, 1023, 1024, 1025, 2049)
CHAIN = 2049


def chain(order):
    """CHAIN collinear points 0.01 apart, indexed ascending, descending or bit-reversed."""
    rank = np.arange(CHAIN)
    if order == "descending":
        rank = rank[::-1]
    elif order == "bit-reversed":
        rank = np.asarray(sorted(range(CHAIN), key=lambda i: int(format(i, "012b")[::-1], 2)))
    P = np.zeros((CHAIN, 3), np.float32)
    P[:, 0] = (rank * 0.01).astype(np.float32)
    P[:, 1] = np.float32(0.5)
    return P


def offset_1000(n, seed=16):
    """A cloud offset by 1 000 with spread 1: the fp32 differences round."""
    return (np.asarray([[1000.0, -1000.0, 1000.0]]) + np.random.RandomState(seed).uniform(-0.5, 0.5, (n, 3))
            ).astype(np.float32)


def blobs_and_chain(cut, seed=17):
    """Two blobs of 300 points joined by a chain of points 0.06 apart (radius 0.1); ``cut`` removes one link."""
    rng = np.random.RandomState(seed)
    ball = rng.normal(size=(600, 3))
    ball = ball / np.linalg.norm(ball, axis=1, keepdims=True) * 0.2 * rng.uniform(0, 1, (600, 1)) ** (1 / 3)
    ball[:300, 0] -= 1.0
    ball[300:, 0] += 1.0
    x = np.arange(-0.84, 0.85, 0.06)
    if cut:
        x = np.delete(x, len(x) // 2)
    link = np.stack([x, np.zeros_like(x), np.zeros_like(x)], 1)
    P = np.concatenate([ball, link]).astype(np.float32)
    return P[rng.permutation(P.shape[0])]


def torus(n, seed, centre=(0, 0, 0), R=1.0, r=0.3, jitter=0.0):
    rng = np.random.RandomState(seed)
    u, v = rng.uniform(0, 2 * np.pi, (2, n))
    P = np.stack([(R + r * np.cos(v)) * np.cos(u), (R + r * np.cos(v)) * np.sin(u), r * np.sin(v)], 1)
    return (P + jitter * rng.normal(size=P.shape) + np.asarray(centre)).astype(np.float32)


def cases():
    """name -> (cloud, radius, min_size)."""
    below = np.nextafter(np.float32(0.25), np.float32(0))
    out = {
        "lattice, radius the spacing": (lattice(11), 0.25, 1),
        "lattice, radius just below the spacing": (lattice(11), float(below), 1),
        "blobs joined by a chain": (blobs_and_chain(False), 0.1, 1),
        "blobs, one link removed": (blobs_and_chain(True), 0.1, 1),
        "copies among random": (copies_among_random(600, 400), 0.05, 1),
        "offset by 1000": (offset_1000(700), 0.08, 1),
        "offset, 1e-4 spacing": (offset_cloud(700), 3e-4, 1),
        "planar": (planar(500), 0.1, 1),
        "collinear": (collinear(300), 0.02, 1),
        "min_size 2": (uniform(1025), between(1025), 2),
        "min_size above the largest": (uniform(1025), between(1025), 1025),
        "torus and a clump": (np.concatenate([torus(900, 31), 0.01 * uniform(30, 32) + np.float32(2.5)]), 0.25, 1),
    }
    for order in ("ascending", "descending", "bit-reversed"):
        out["chain %s" % order] = (chain(order), 0.011, 1)
    for n in SIZES:
        P = uniform(n)
        out["uniform %d, every point alone" % n] = (P, ALONE, 1)
        out["uniform %d, between" % n] = (P, between(n), 1)
        out["uniform %d, one component" % n] = (P, ONE, 1)
    return out


BAD_RADII = (0.0, float("nan"), float("inf"), 1e-30, -1.0, 1e30)      # 1e-30: r2 underflows; 1e30: it overflows


# ---------------------------------------------------------------------------------------------
# the host-compiled header
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return native.build_harness(tmp_path_factory.mktemp("clh"), "clh", SOURCE)


def host_cluster(lib, batch, radii, min_size=1, order=0, want_report=False):
    n = [c.shape[0] for c in batch]
    off = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
    S, total = len(batch), int(off[-1])
    P = np.ascontiguousarray(np.concatenate([c.reshape(-1, 3) for c in batch]), np.float32)
    rad = np.asarray(radii, np.float32)
    label, count, first = (np.full(total, -9, np.int32) for _ in range(3))
    ncomp, ndrop = np.full(S, -9, np.int32), np.full(S, -9, np.int32)
    report = np.zeros(8, np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    rc = lib.clh_cluster(p(P), p(off), S, total, p(rad), int(min_size), order, p(label), p(ncomp), p(count), p(first),
                         p(ndrop), p(report))
    assert rc == lib.clh_launches(max(n)) and report[0] == 1, report      # the schedule sufficed
    out = (label, ncomp, count, first, ndrop)
    return (out, report) if want_report else out


def equal(got, want):
    return all(same(np.asarray(g), np.asarray(w, np.asarray(g).dtype)) for g, w in zip(got, want))


def one(want):
    """The result of cluster_numpy in the shape of a batch of one."""
    return want[0], [want[1]], want[2], want[3], [want[4]]


@pytest.fixture(scope="module")
def reference():
    """name -> cluster_numpy of the case: computed once, shared, never changed."""
    return {name: cluster_numpy(*case) for name, case in cases().items()}


@pytest.mark.parametrize("name", sorted(cases()))
def test_the_simulated_schedule_equals_the_definition(harness, reference, name):
    P, r, min_size = cases()[name]
    want = reference[name]
    n = P.shape[0]
    for order in (0, 1):
        got, report = host_cluster(harness, [P], [r], min_size, order, want_report=True)
        assert equal(got, one(want)), (name, order)
        assert report[1] < report[2] and report[3] <= report[4]             # the bounds of the header hold
    check_properties(P, want)
    C = want[1]
    if "alone" in name or name == "lattice, radius just below the spacing":
        assert C == n and (want[2] == 1).all()
    if "one component" in name or name == "lattice, radius the spacing" or name.startswith("chain"):
        assert C == 1 and want[2][0] == n
    if "one component" in name:
        assert report[7] == 1 and report[5] == 1                             # one cell: the cube covers it at ring 0
    if "between" in name and n >= 1023:
        assert 100 <= C < n and want[2][:C].max() > 3                   # some hundred components
    if name == "blobs joined by a chain":
        assert C == 1
    if name == "blobs, one link removed":
        assert C == 2 and abs(int(want[2][0]) - int(want[2][1])) <= 1
    if name == "min_size 2":
        assert 0 < C and want[4] > 0 and (want[2][:C] >= 2).all()
    if name == "min_size above the largest":
        assert C == 0 and want[4] == n and (want[0] == -1).all()
    if name == "torus and a clump":
        assert C == 2 and sorted(want[2][:2].tolist()) == [30, 900]
    if name == "planar" or name.startswith("chain"):                         # (collinear runs askew: three dimensions)
        dim, h = (ctypes.c_int * 3)(), ctypes.c_float()
        harness.clh_grid(P.ctypes.data_as(ctypes.c_void_p), n, ctypes.c_float(r), dim, ctypes.byref(h))
        assert min(dim) == 1 < max(dim)                                      # a grid dimension collapsed
    if name.startswith("chain"):
        assert report[6] >= 1


def test_the_grid_keeps_the_cell_edge_at_the_radius(harness):
    harness.clh_grid.restype = ctypes.c_int
    dim, h = (ctypes.c_int * 3)(), ctypes.c_float()
    P = uniform(2049)
    for r in (0.05, 0.11, 0.3, 0.7, 1.0, 1.99):
        cells = harness.clh_grid(P.ctypes.data_as(ctypes.c_void_p), 2049, ctypes.c_float(r), dim, ctypes.byref(h))
        assert 1 <= cells <= 8 ** 3 and max(dim) <= 8                          # kg_resolution(2049, 4) = 8
        assert max(dim) == 1 or h.value >= np.float32(r)


def test_a_permutation_permutes_the_partition_and_nothing_else(harness, reference):
    for name in ("uniform 2049, between", "copies among random", "offset by 1000", "blobs, one link removed",
                 "min_size 2", "chain bit-reversed"):
        P, r, min_size = cases()[name]
        want = partition(P, reference[name][0])
        for seed in (1, 2):
            Q = P[np.random.RandomState(seed).permutation(P.shape[0])]
            ref = cluster_numpy(Q, r, min_size)
            assert partition(Q, ref[0]) == want, name
            assert equal(host_cluster(harness, [Q], [r], min_size, seed - 1), one(ref)), name


def ragged_batch():
    """clouds, radii: 1 300 points, an empty cloud, one point, a NaN cloud in the middle, five points, an inf cloud, a
    lattice, a cloud whose radius has no fp32 square; a different radius per cloud."""
    nan, inf = uniform(40, 3), uniform(1031, 4)
    nan[11, 1], inf[1026, 0] = np.nan, -np.inf
    clouds = [uniform(1300, 5), np.zeros((0, 3), np.float32), uniform(1, 8), nan, uniform(5, 6), inf, lattice(5),
              uniform(70, 7)]
    radii = [0.12, 0.3, 0.2, 0.1, 0.9, 0.15, 0.25, 1e-30]
    return clouds, radii


def test_a_ragged_batch_with_empty_short_and_non_finite_clouds(harness):
    clouds, radii = ragged_batch()
    for min_size in (1, 3):
        want = cluster_numpy_batch(clouds, radii, min_size)
        assert want[1].tolist()[1:4] == [0, 1 if min_size == 1 else 0, -1] and want[1][5] == -1 and want[1][7] == -2
        assert want[1][0] > 50 and want[1][6] == 1
        for order in (0, 1):
            assert equal(host_cluster(harness, clouds, radii, min_size, order), want)
        o = 0
        for c, P in enumerate(clouds):                                       # every cloud alone gives what it gives here
            alone = host_cluster(harness, [P], [radii[c]], min_size)
            n = P.shape[0]
            assert alone[1][0] == want[1][c] and alone[4][0] == want[4][c]
            assert equal([alone[t] for t in (0, 2, 3)], [want[t][o:o + n] for t in (0, 2, 3)])
            o += n


def test_statuses(harness):
    P = uniform(65)
    Q = P.copy()
    Q[7, 2] = np.inf
    for bad in BAD_RADII:
        assert radius_status(bad) == -2
        got = host_cluster(harness, [P, Q, np.zeros((0, 3), np.float32)], [bad, bad, bad])
        assert got[1].tolist() == [-2, -1, -2] and (got[0] == -1).all() and (got[2] == -1).all()
        assert got[4].tolist() == [65, 65, 0]
        assert equal(got, cluster_numpy_batch([P, Q, np.zeros((0, 3), np.float32)], [bad] * 3))
    got = host_cluster(harness, [Q], [0.3])
    assert got[1].tolist() == [-1] and equal(got, one(cluster_numpy(Q, 0.3)))


def test_the_program_under_the_sanitizers_over_the_case_list(tmp_path, reference):
    """The same file with its main, built with -fsanitize=address,undefined (the runtimes linked into the program) and
    run once over its own list (both orders of arrival against a brute force) and once over every case of ``cases()``
    from a file, in both orders.  It runs in the environment it finds: nothing is preloaded or set for it."""
    exe = os.path.join(str(tmp_path), "cluster_host")
    subprocess.run(native.GXX + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                 "-static-libasan", "-static-libubsan", "-o", exe, SOURCE], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and " 0 differences" in run.stdout and run.stderr == "", (run.stdout, run.stderr)
    names = sorted(cases())
    path = tmp_path / "clouds.txt"
    with open(path, "w") as f:
        for name in names:
            P, r, min_size = cases()[name]
            f.write("%d %.9g %d\n" % (P.shape[0], np.float32(r), min_size))
            f.write("".join("%.9g %.9g %.9g\n" % tuple(p) for p in P.tolist()))
    run = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-2000:]
    want = []
    for name in names:
        want += [reference[name][1]] + reference[name][0].tolist()
    assert [int(v) for v in run.stdout.split()] == want


# ---------------------------------------------------------------------------------------------
# the export, the schedule, the workspace and the argument checks, which run before anything touches a GPU
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    return native.load_raw(NAMES)


def launches(max_n):
    """The header's formula: 4 + (ceil(log2 max_n) + 1) (2 + ceil(log_64 max_n)) + 3, in integers."""
    rounds = 1 + max(0, (max_n - 1).bit_length())
    passes, reach = 1, 64
    while reach < max_n:
        reach, passes = reach * 64, passes + 1
    return 4 + rounds * (2 + passes) + 3


def test_the_entry_points_are_exported_and_bound(lib, harness):
    from parsenet_codebase_amd import _lib
    v, i, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    assert _lib.SIGNATURES["pn_cluster_f32"] == (i, [v, v, i, i, i, v, i, v, v, v, v, v, v, ll, v])
    assert _lib.SIGNATURES["pn_cluster_workspace_bytes"] == (ll, [ll, i])
    assert _lib.SIGNATURES["pn_cluster_launches"] == (i, [i])
    assert lib.pn_abi_version() == 23 == _lib.CONSTANTS["PN_ABI_VERSION"]                   # added symbols only
    assert all(hasattr(_lib.load(), n) for n in NAMES)
    for max_n, want in ((1, 10), (2, 13), (1024, 51), (10240, 82), (2 ** 31 - 1, 263)):
        assert lib.pn_cluster_launches(max_n) == launches(max_n) == harness.clh_launches(max_n) == want, max_n
    assert lib.pn_cluster_launches(0) == lib.pn_cluster_launches(-5) == launches(1)
    assert harness.clh_rounds(2 ** 31 - 1) == 32 == harness.clh_constant(1)
    assert harness.clh_passes(2 ** 31 - 1) == 6 < harness.clh_constant(2)
    w = lib.pn_cluster_workspace_bytes
    words = harness.clh_constant(3)
    for total, S in ((1, 1), (1024, 3), (10 ** 6, 7), (2 ** 31 - 1, 1)):
        assert w(total, S) == 56 * total + 36 * S + 4 * words + 16, (total, S)   # the formula of the header
    assert 4 * words + 16 == 1296
    assert w(2 ** 31, 1) == 0 and w(-1, 1) == 0 and w(10, -1) == 0


ARGS = ("pts", "off", "S", "total", "max_n", "radius", "min_size", "label", "ncomp", "count", "first", "ndrop", "ws",
        "ws_bytes", "stream")


def raw_call(lib, **over):
    """pn_cluster_f32 with plausible arguments (never dereferenced by a call that is refused), some replaced."""
    a = dict(pts=64, off=64, S=1, total=10, max_n=10, radius=64, min_size=1, label=64, ncomp=64, count=None, first=None,
             ndrop=None, ws=64, ws_bytes=lib.pn_cluster_workspace_bytes(10, 1), stream=None)
    a.update(over)
    return lib.pn_cluster_f32(*[a[n] for n in ARGS])


def test_invalid_arguments_are_refused_before_any_launch(lib):
    """(No GPU is needed to get here: a refused call, and one with nothing to do, launch nothing.)"""
    from parsenet_codebase_amd import _lib
    err = _lib.CONSTANTS["PN_ERR_ARG"]
    need = lib.pn_cluster_workspace_bytes(10, 1)
    for over, word in ((dict(S=-1), b"S=-1"), (dict(total=-1), b"total=-1"), (dict(max_n=-1), b"max_n=-1"),
                       (dict(min_size=0), b"min_size=0"), (dict(min_size=-3), b"min_size=-3"),
                       (dict(pts=None), b"null"), (dict(off=None), b"null"), (dict(radius=None), b"null"),
                       (dict(label=None), b"null"), (dict(ncomp=None), b"null"), (dict(ws=None), b"null"),
                       (dict(ws_bytes=need - 1), b"workspace"), (dict(ws_bytes=0), b"workspace")):
        assert raw_call(lib, **over) == err, over
        assert b"pn_cluster_f32" in lib.pn_last_error() and word in lib.pn_last_error(), (over, lib.pn_last_error())
    assert raw_call(lib, S=0) == 0 and raw_call(lib, total=0) == 0
    assert raw_call(lib, S=0, pts=None, label=None, ncomp=None, ws=None, ws_bytes=0) == 0
    assert raw_call(lib, total=0, pts=None, radius=None, ws=None, ws_bytes=0) == 0
    assert raw_call(lib, S=0, min_size=0) == err                               # the arguments come first


def test_python_argument_checks_need_no_gpu():
    import torch
    from parsenet_codebase_amd import cleaning, kernels
    P = torch.zeros(8, 3)
    off = torch.tensor([0, 8], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="MI355X only"):
        kernels.cluster_ragged(P, off, torch.ones(1))
    for radius in (0.1, [0.1], None, np.ones(1, np.float32)):                  # the named errors come first
        with pytest.raises(TypeError, match="cluster_ragged: radius must be a tensor"):
            kernels.cluster_ragged(P, off, radius)
    for min_size in (0, "2", 1.5, None, True, 2 ** 31):
        with pytest.raises(ValueError, match="cluster_ragged: min_size must be"):
            kernels.cluster_ragged(P, off, torch.ones(1), min_size)
    with pytest.raises(ValueError, match="cluster_ragged: want holds"):
        kernels.cluster_ragged(P, off, torch.ones(1), 1, want=("rep",))
    for fn in (cleaning.euclidean_clusters, cleaning.split_clusters, cleaning.keep_largest):
        with pytest.raises(RuntimeError, match="MI355X only"):
            fn(P, radius=0.1)
        for radius in (0, -1, float("inf"), float("nan"), True, "a", 1e-60, [0.0], None):
            with pytest.raises(ValueError, match="radius must be"):
                fn(P, radius=radius)
        for radius in ([0.1], [0.1, 0.2, 0.3], np.asarray([0.1, 0.2, 0.3])):
            with pytest.raises(ValueError, match="radius holds one number per cloud"):
                fn([P, P], radius=radius)
        with pytest.raises(ValueError, match="radius must be"):
            fn([P, P], radius=[0.1, 0.0])
    for fn in (cleaning.euclidean_clusters, cleaning.split_clusters):
        for min_size in (0, -1, 1.5, True, "2", None, 2 ** 31):
            with pytest.raises(ValueError, match="min_size must be"):
                fn(P, radius=0.1, min_size=min_size)
    for order in ("Size", None, 0, "largest"):
        with pytest.raises(ValueError, match="order must be"):
            cleaning.split_clusters(P, radius=0.1, order=order)
