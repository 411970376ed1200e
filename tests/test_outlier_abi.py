"""CPU-side checks of the statistical outlier removal: csrc/outlier_math.h compiled for the host into a serial
restatement of the kernels' schedule (tests/native/outlier_host.cpp: tile table, per-point statistic, the summation tree,
the per-cloud sequential sums, mask, counts and compaction) against ``outlier_numpy``, an independent numpy restatement
of the definition and the tree — avg, stats, keep, kept and index equal bit for bit, in both tile orders —, the accuracy
of the tree against math.fsum, the stand-alone program, the export of csrc/outlier.hip and its argument checks, and the
argument checks of ``cleaning``."""
import ctypes
import math
import subprocess

import numpy as np
import pytest

from tests.helpers import native
from tests.helpers.native import ROOT      # noqa: F401  (tests/test_outlier_gpu.py takes it from here)
from tests.test_knn3_grid_abi import brute_dist, copies_among_random, cube_and_far_point, identical, lattice
from tests.test_point_normals_abi import knn3

SOURCE = native.source("outlier_host.cpp")
NAMES = ("pn_outlier_stat_f32", "pn_outlier_workspace_bytes", "pn_outlier_launches")
TILE = 1024      # OL_TILE of csrc/outlier_math.h (test_the_tile_is_the_one_the_tests_assume)
LAUNCHES = 6
SIZES = (1, 2, 19, 20, 21, 63, 64, 65, 1023, 1024, 1025, 2049)


# ---------------------------------------------------------------------------------------------
# the definition and the tree, in numpy (shared with tests/test_outlier_gpu.py)
# ---------------------------------------------------------------------------------------------
def tree_sum(v):
    """SUM of csrc/outlier_math.h over the fp64 terms of one cloud."""
    n = v.shape[0]
    tiles = -(-n // TILE)
    s = np.zeros(tiles * TILE, np.float64)
    s[:n] = v
    s = s.reshape(tiles, 4, 256)
    s = (((s[:, 0] + s[:, 1]) + s[:, 2]) + s[:, 3]).reshape(tiles, 4, 64)
    for h in (32, 16, 8, 4, 2, 1):
        s = s + s[..., np.arange(64) ^ h]
    w = s[..., 0]
    total = np.float64(0.0)
    for t in ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]:
        total = total + t
    return total


def outlier_numpy(dist, k, std_ratio):
    """One cloud by the definition: (avg (n) fp64, stats (3) fp64, keep (n) uint8, kept, index (n) int32)."""
    d = np.ascontiguousarray(dist, np.float32).reshape(-1, k)
    n = d.shape[0]
    kc = min(k, n)
    with np.errstate(all="ignore"):
        s = np.zeros(n, np.float64)
        for j in range(kc):
            s = s + d[:, j].astype(np.float64)
        a = s / np.float64(kc)
        valid = a > 0
        mean = tree_sum(np.where(valid, a, np.where(np.isnan(a), np.nan, 0.0))) / np.float64(n)
        if np.isnan(mean):
            a = np.full(n, np.nan)                      # a NaN statistic poisons its cloud
        dev = a - mean
        dev = tree_sum(np.where(valid, dev * dev, np.where(np.isnan(a), np.nan, 0.0)))
        std = np.sqrt(dev / np.float64(n - 1)) if n > 1 else np.float64(0.0)
        thr = mean + np.float64(std_ratio) * std
        keep = valid & (a < thr)
    index = np.full(n, -1, np.int32)
    index[:keep.sum()] = np.flatnonzero(keep)
    return a, np.asarray([mean, std, thr], np.float64), keep.astype(np.uint8), int(keep.sum()), index


def outlier_numpy_batch(dists, k, std_ratio):
    """A ragged batch: (avg (total), stats (S,3), keep (total), kept (S) int32, index (total))."""
    out = [outlier_numpy(d, k, std_ratio) for d in dists]
    return (np.concatenate([o[0] for o in out]), np.stack([o[1] for o in out]), np.concatenate([o[2] for o in out]),
            np.asarray([o[3] for o in out], np.int32), np.concatenate([o[4] for o in out]))


def same(a, b):
    """Exact equality of two arrays; NaN equals NaN for the floating-point ones."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


OUTPUTS = ("avg", "stats", "keep", "kept", "index")


def neighbour_dist(P, k):
    """(n,k) fp32: what knn3_ragged / knn3_grid return as dist for one cloud — NaN rows if it holds a non-finite
    coordinate."""
    P = np.ascontiguousarray(P, np.float32).reshape(-1, 3)
    if not np.isfinite(P).all():
        return np.full((P.shape[0], k), np.nan, np.float32)
    if P.shape[0] == 0:
        return np.zeros((0, k), np.float32)
    return brute_dist(P, knn3(P, k))


def with_strays(n, seed, strays=3):
    """n uniform points in the unit cube, ``strays`` of them pushed 3 .. 5 units out."""
    rng = np.random.RandomState(seed)
    P = rng.uniform(0, 1, (n, 3)).astype(np.float32)
    m = min(strays, n // 8)
    P[rng.permutation(n)[:m]] += rng.uniform(3, 5, (m, 3)).astype(np.float32)
    return P


def equal_statistic_cloud():
    """The eight corners of a cube: every point has the same neighbour distances, hence the same statistic."""
    return np.asarray([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float32)


# ---------------------------------------------------------------------------------------------
# the host-compiled header
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return native.build_harness(tmp_path_factory.mktemp("olh"), "olh", SOURCE)


def host_stat(lib, dists, k, std_ratio, order=0, want_index=True, sums=None):
    sizes = [d.shape[0] for d in dists]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    S, total = len(dists), int(off[-1])
    D = np.ascontiguousarray(np.concatenate([d.reshape(-1, k) for d in dists]), np.float32)
    avg, stats = np.full(total, -7.0), np.full((S, 3), -7.0)
    keep, kept, index = np.full(total, 7, np.uint8), np.full(S, -7, np.int32), np.full(total, -7, np.int32)
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    lib.olh_stat.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                             ctypes.c_double, ctypes.c_int] + [ctypes.c_void_p] * 6
    rc = lib.olh_stat(p(D), p(off), S, total, k, std_ratio, order, p(avg), p(stats), p(keep), p(kept),
                      p(index if want_index else None), p(sums))
    assert rc == (LAUNCHES if total else 0)
    return avg, stats, keep, kept, index


def check_host(harness, dists, k, std_ratio, what):
    want = outlier_numpy_batch(dists, k, std_ratio)
    for order in (0, 1):
        got = host_stat(harness, dists, k, std_ratio, order)
        for name, g, w in zip(OUTPUTS, got, want):
            assert same(g, w), "%s: %s differs (k = %d, ratio = %g, order %d)" % (what, name, k, std_ratio, order)
    return want


def check_one(harness, dist, k, std_ratio, what):
    """``check_host`` on one cloud -> (avg, stats (3), keep, kept as an int, index)."""
    avg, stats, keep, kept, index = check_host(harness, [dist], k, std_ratio, what)
    return avg, stats[0], keep, int(kept[0]), index


def test_the_tile_is_the_one_the_tests_assume(harness):
    assert harness.olh_tile() == TILE and harness.olh_launches() == LAUNCHES


@pytest.mark.parametrize("n", SIZES)
def test_the_restated_schedule_equals_the_definition(harness, n):
    P = with_strays(n, n)
    for k in (1, 8, 20, 64):
        dist = neighbour_dist(P, k)
        for ratio in (0.0, 0.5, 2.0):
            avg, stats, keep, kept, index = check_one(harness, dist, k, ratio, "n = %d" % n)
            assert kept == keep.sum() and (np.diff(index[:kept]) > 0).all() and (index[kept:] == -1).all()
    if n >= 64:
        assert 0 < kept < n                         # k = 64, ratio 2: the statistic decides, neither all nor nothing
    if n == 1:
        assert kept == 0 and stats.tolist() == [0.0, 0.0, 0.0]


def test_special_clouds(harness):
    k = 20
    avg, stats, keep, kept, _ = check_one(harness, neighbour_dist(identical(50), k), k, 2.0, "identical")
    assert (avg == 0).all() and kept == 0 and not keep.any() and stats.tolist() == [0.0, 0.0, 0.0]
    P = copies_among_random(600, 400)
    copies = (P == np.asarray([0.125, -0.25, 0.375], np.float32)).all(1)
    avg, _, keep, kept, _ = check_one(harness, neighbour_dist(P, k), k, 2.0, "copies among random")
    assert copies.sum() == 600 and (avg[copies] == 0).all() and not keep[copies].any() and 0 < kept <= 400
    check_one(harness, neighbour_dist(lattice(11), 7), 7, 1.0, "lattice")
    P = cube_and_far_point(1000)
    _, _, keep, kept, _ = check_one(harness, neighbour_dist(P, k), k, 2.0, "cube and a far point")
    assert not keep[1000 // 3] and kept > 900
    # every statistic equal: std = 0, thr = mean, and the strict comparison keeps nothing
    avg, stats, keep, kept, index = check_one(harness, neighbour_dist(equal_statistic_cloud(), 4), 4, 2.0, "corners")
    assert (avg == avg[0]).all() and avg[0] > 0 and stats[1] == 0 and stats[2] == stats[0] == avg[0]
    assert kept == 0 and (index == -1).all()


def test_a_ragged_batch_with_empty_short_and_non_finite_clouds(harness):
    k = 20
    nan, inf = with_strays(40, 1), with_strays(TILE + 7, 2)
    nan[11, 1], inf[TILE + 2, 0] = np.nan, -np.inf
    batch = [with_strays(TILE + 300, 3), np.zeros((0, 3), np.float32), nan, with_strays(3, 4), inf, with_strays(500, 5)]
    dists = [neighbour_dist(P, k) for P in batch]
    want = check_host(harness, dists, k, 1.0, "ragged")
    avg, stats, keep, kept, index = want
    assert kept[[1, 2, 4]].tolist() == [0, 0, 0] and 1 <= kept[3] <= 3 and kept[0] > 1000 and kept[5] > 400
    assert np.isnan(stats[[2, 4]]).all() and np.isnan(stats[1, [0, 2]]).all() and stats[1, 1] == 0
    o = np.concatenate([[0], np.cumsum([P.shape[0] for P in batch])])
    assert np.isnan(avg[o[2]:o[3]]).all() and np.isnan(avg[o[4]:o[5]]).all() and not keep[o[2]:o[3]].any()
    assert (avg[o[3]:o[4]] > 0).all() and same(avg[o[3]:o[4]], outlier_numpy(dists[3][:, :3], 3, 1.0)[0])   # k_c = 3
    # every cloud alone gives what it gives in the batch
    for c, d in enumerate(dists):
        alone = host_stat(harness, [d], k, 1.0)
        if d.shape[0] == 0:
            continue                                                             # nothing is launched, nothing written
        assert same(alone[0], avg[o[c]:o[c + 1]]) and same(alone[1][0], stats[c]) and same(alone[2], keep[o[c]:o[c + 1]])
        assert alone[3][0] == kept[c] and same(alone[4], index[o[c]:o[c + 1]])
    # without index: the other outputs are the same
    got = host_stat(harness, dists, k, 1.0, want_index=False)
    assert all(same(g, w) for g, w in zip(got[:4], want[:4])) and (got[4] == -7).all()


def test_the_tree_is_as_accurate_as_its_depth(harness):
    """mean and the deviation sum against math.fsum on the same a: (13 + tiles) 2^-52 relative (csrc/outlier_math.h)."""
    for n in (65, 1025, 2049):
        k = 20
        sums = np.zeros((1, 2))
        a, stats, _, _, _ = host_stat(harness, [neighbour_dist(with_strays(n, n), k)], k, 2.0, sums=sums)
        bound = (13 + -(-n // TILE)) * 2.0 ** -52
        assert (a > 0).all()                                              # every term is the statistic itself
        mean = math.fsum(a.tolist()) / n
        assert abs(stats[0, 0] - mean) <= bound * mean and stats[0, 0] == sums[0, 0] / n
        terms = (a - stats[0, 0]) * (a - stats[0, 0])
        dev = math.fsum(terms.tolist())
        assert abs(sums[0, 1] - dev) <= bound * dev and sums[0, 1] == tree_sum(terms)
        assert stats[0, 1] == np.sqrt(sums[0, 1] / (n - 1))


def test_the_program_checks_itself(harness, tmp_path):
    exe = native.build_program(tmp_path, "outlier_host", SOURCE)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and " 0 differences" in run.stdout, run.stdout


# ---------------------------------------------------------------------------------------------
# the export and the argument checks, which run before anything touches a GPU
# ---------------------------------------------------------------------------------------------
def load_raw():
    return native.load_raw(NAMES)


@pytest.fixture(scope="module")
def lib():
    return load_raw()


def test_the_entry_points_are_exported_and_bound(lib):
    from parsenet_codebase_amd import _lib
    v, i, ll, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_double
    assert _lib.SIGNATURES["pn_outlier_stat_f32"] == (i, [v, v, i, i, i, d, v, v, v, v, v, v, ll, v])
    assert _lib.SIGNATURES["pn_outlier_workspace_bytes"] == (ll, [ll, i])
    assert _lib.SIGNATURES["pn_outlier_launches"] == (i, [])
    assert lib.pn_abi_version() == 23 == _lib.CONSTANTS["PN_ABI_VERSION"]                   # added symbols only
    assert all(hasattr(_lib.load(), n) for n in NAMES)
    assert lib.pn_outlier_launches() == LAUNCHES
    w = lib.pn_outlier_workspace_bytes
    # linear in total, known from (total, S) alone
    assert w(0, 0) >= 0 and w(1000, 3) >= 20 * 3
    m = 1000 * TILE                                           # 20 bytes per tile of 1 024 points: steps of a whole tile
    assert w(2 * m, 3) - w(m, 3) == w(3 * m, 3) - w(2 * m, 3) == 20 * 1000
    assert w(2 ** 40, 1) > 2 ** 32                                                           # long long, not int
    assert w(-1, 1) == 0 and w(1, -1) == 0


ARGS = ("dist", "off", "S", "total", "k", "std_ratio", "avg", "stats", "keep", "kept", "index", "ws", "ws_bytes",
        "stream")


def raw_call(lib, **over):
    """pn_outlier_stat_f32 with plausible arguments (never dereferenced by a call that is refused), some replaced."""
    a = dict(dist=64, off=64, S=1, total=10, k=8, std_ratio=2.0, avg=64, stats=64, keep=64, kept=64, index=None, ws=64,
             ws_bytes=lib.pn_outlier_workspace_bytes(10, 1), stream=None)
    a.update(over)
    return lib.pn_outlier_stat_f32(*[a[n] for n in ARGS])


def check_invalid_arguments(lib, **real):
    """k out of range, S or total < 0, total * k >= 2^31, a negative or non-finite std_ratio, a null required pointer,
    a short workspace: PN_ERR_ARG, the message naming the function; nothing to do: 0."""
    from parsenet_codebase_amd import _lib
    err = _lib.CONSTANTS["PN_ERR_ARG"]
    need = lib.pn_outlier_workspace_bytes(real.get("total", 10), real.get("S", 1))
    for over in (dict(k=0), dict(k=65), dict(k=-1), dict(S=-1), dict(total=-1), dict(total=2 ** 31 // 8, k=8),
                 dict(total=2 ** 31 - 1, k=64), dict(std_ratio=-0.5), dict(std_ratio=float("nan")),
                 dict(std_ratio=float("inf")), dict(dist=None), dict(off=None), dict(avg=None), dict(stats=None),
                 dict(keep=None), dict(kept=None), dict(ws=None), dict(ws_bytes=need - 1), dict(ws_bytes=0)):
        assert raw_call(lib, **dict(real, **over)) == err, over
        assert b"pn_outlier_stat_f32" in lib.pn_last_error(), (over, lib.pn_last_error())
    assert raw_call(lib, **dict(real, total=0)) == 0
    assert raw_call(lib, **dict(real, S=0)) == 0
    assert raw_call(lib, **dict(real, total=0, dist=None, avg=None, keep=None, ws=None, ws_bytes=0)) == 0


def test_invalid_arguments_are_refused_before_any_launch(lib):
    """(No GPU is needed to get here: a refused call, and one with nothing to do, launch nothing.)"""
    check_invalid_arguments(lib)


def test_python_argument_checks_need_no_gpu():
    import torch
    from parsenet_codebase_amd import cleaning, kernels
    from parsenet_codebase_amd.ragged import Clouds
    P = torch.zeros(8, 3)
    for k in (0, 65, -1, 2.5, True, "3", None):
        for call in (cleaning.outlier_statistic, cleaning.remove_outliers):
            with pytest.raises(ValueError, match="k must be"):
                call(P, k=k)
    for ratio in (-0.1, float("nan"), float("inf"), "2", None, True):
        for call in (cleaning.outlier_statistic, cleaning.remove_outliers):
            with pytest.raises(ValueError, match="std_ratio must be"):
                call(P, std_ratio=ratio)
    for call in (cleaning.outlier_statistic, cleaning.remove_outliers):
        with pytest.raises(RuntimeError, match="MI355X only"):
            call(P)
    # the checks behind the device check, on the shape logic of a Clouds that skips it
    clouds = Clouds([torch.zeros(5, 3), torch.zeros(3, 3)], "test", on_gpu=False)
    with pytest.raises(ValueError, match="search must be"):
        cleaning._statistic(clouds, 20, 2.0, "kd-tree", "test", False)
    big = Clouds(torch.zeros(kernels.KNN3_MAX_POINTS + 1, 3), "test", on_gpu=False)
    with pytest.raises(ValueError, match="search=\"grid\" lifts the limit"):
        cleaning._statistic(big, 20, 2.0, None, "test", False)
    with pytest.raises(ValueError, match="same layout"):
        clouds.beside(torch.zeros(8), "test", "a per-point array")
    with pytest.raises(RuntimeError, match="MI355X only"):
        kernels.outlier_stat(torch.zeros(8, 4), torch.zeros(2, dtype=torch.int32), 4, 2.0)
    # restore is index arithmetic and runs anywhere
    out = cleaning.restore(torch.tensor([5, 6, 7]), torch.tensor([0, 2, 3]), 5, -1)
    assert out.tolist() == [5, -1, 6, 7, -1] and out.dtype == torch.int64
    rows = cleaning.restore(torch.ones(2, 3), torch.tensor([1, 2]), 4, 0.5)
    assert rows.tolist() == [[0.5] * 3, [1.0] * 3, [1.0] * 3, [0.5] * 3]
    both = cleaning.restore([torch.tensor([1]), torch.tensor([2, 3])], [torch.tensor([0]), torch.tensor([0, 1])], [2, 2], 0)
    assert [b.tolist() for b in both] == [[1, 0], [2, 3]]
    assert cleaning.restore(torch.zeros(0), torch.zeros(0, dtype=torch.int64), 3, -1.0).tolist() == [-1.0] * 3
    for index in ([0, 5], [-1, 2]):
        with pytest.raises(ValueError, match="outside the 5 points"):
            cleaning.restore(torch.tensor([1, 2]), torch.tensor(index), 5, -1)
    with pytest.raises(ValueError, match="index \\(kept,\\)"):
        cleaning.restore(torch.tensor([1, 2, 3]), torch.tensor([0, 1]), 5, -1)
