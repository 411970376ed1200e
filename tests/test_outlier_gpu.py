"""GPU checks of the statistical outlier removal (csrc/outlier.hip, parsenet_codebase_amd/cleaning.py): avg, stats, keep,
kept and index equal to the numpy restatement of the definition (tests.test_outlier_abi.outlier_numpy) at every size
around the wave and the tile, for every k and ratio, on clouds that do not start on a tile, alone, in a batch and on a
second run, in the three layouts, with either neighbour search, with non-finite, empty, short and coincident clouds, on
a hundred thousand points with strays; remove_outliers and restore with their host reads counted; the masks against
the project's fp64 oracle outside a band that follows from the fp32 distances; the purpose (farthest-point sampling
stops picking strays); the raw ABI.  Apart from the oracle's band there is no tolerance in this file."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests.test_knn3_grid_abi import identical
from tests.test_outlier_abi import (OUTPUTS, ROOT, SIZES, TILE, check_invalid_arguments, load_raw, neighbour_dist,
                                    outlier_numpy, outlier_numpy_batch, raw_call, same, with_strays)

pytestmark = pytest.mark.gpu


def _stat(gpu, dists, k, ratio, want_index=True):
    """kernels.outlier_stat on a ragged batch of numpy distances -> (avg, stats, keep, kept, index) as numpy."""
    from parsenet_codebase_amd import kernels as K
    sizes = [d.shape[0] for d in dists]
    flat = torch.from_numpy(np.ascontiguousarray(np.concatenate([d.reshape(-1, k) for d in dists]), np.float32)).to(gpu)
    off = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)).to(gpu)
    out = K.outlier_stat(flat, off, k, ratio, want_index=want_index)
    assert out[2].dtype == torch.bool
    return tuple(o.cpu().numpy().astype(np.uint8) if o.dtype == torch.bool else o.cpu().numpy() for o in out)


def _check(gpu, dists, k, ratio, what=""):
    got, want = _stat(gpu, dists, k, ratio), outlier_numpy_batch(dists, k, ratio)
    for name, g, w in zip(OUTPUTS, got, want):
        assert same(g, w), "%s: %s differs (k = %d, ratio = %g)" % (what, name, k, ratio)
    return got


@pytest.fixture(scope="module")
def dist64():
    """n -> the (n,64) distances of ``with_strays(n, n)``, computed once: for n >= 64 the first k columns are the
    distances of the k nearest."""
    cache = {}

    def get(n):
        if n not in cache:
            cache[n] = neighbour_dist(with_strays(n, n), 64)
        return cache[n]
    return get


def _dist(dist64, n, k):
    return np.ascontiguousarray(dist64(n)[:, :k]) if n >= 64 else neighbour_dist(with_strays(n, n), k)


@pytest.mark.parametrize("n", SIZES + (3 * TILE + 7,))
def test_every_size_k_and_ratio(gpu, dist64, n):
    for k in (1, 8, 20, 64):
        dist = _dist(dist64, n, k)
        for ratio in (0.0, 0.5, 2.0):
            _check(gpu, [dist], k, ratio, what="n = %d" % n)


def test_alone_in_a_batch_off_the_tile_grid_and_on_a_second_run(gpu, dist64):
    k = 20
    five = [_dist(dist64, 1025, k), np.zeros((0, k), np.float32), _dist(dist64, 19, k), _dist(dist64, 2049, k),
            _dist(dist64, 65, k)]
    for batch in ([five[2], five[3]], five, [five[1], five[4], five[1], five[0]]):
        starts = np.cumsum([0] + [d.shape[0] for d in batch])[:-1]
        assert any(s % TILE and d.shape[0] > TILE for s, d in zip(starts, batch))      # tiles cut by the cloud
        got = _check(gpu, batch, k, 1.0, what="batch of %d" % len(batch))
        assert all(same(a, b) for a, b in zip(got, _stat(gpu, batch, k, 1.0))), "a second run changed a result"
        o = 0
        for c, d in enumerate(batch):
            n = d.shape[0]
            if n:
                alone = _stat(gpu, [d], k, 1.0)
                assert same(alone[0], got[0][o:o + n]) and same(alone[1][0], got[1][c])
                assert same(alone[2], got[2][o:o + n]) and alone[3][0] == got[3][c] and same(alone[4], got[4][o:o + n])
            o += n
    without = _stat(gpu, five, k, 1.0, want_index=False)
    assert len(without) == 4 and all(same(a, b) for a, b in zip(without, _stat(gpu, five, k, 1.0)[:4]))


def _np(x):
    return x.cpu().numpy().astype(np.uint8) if x.dtype == torch.bool else x.cpu().numpy()


def test_the_three_layouts_agree(gpu):
    from parsenet_codebase_amd.cleaning import outlier_statistic
    P = np.stack([with_strays(1500, 5), with_strays(1500, 6)])
    T = torch.from_numpy(P).to(gpu)
    batch = outlier_statistic(T, k=8, std_ratio=1.0, return_stats=True)
    assert [tuple(b.shape) for b in batch] == [(2, 1500), (2, 1500), (2, 3)]
    assert [b.dtype for b in batch] == [torch.bool, torch.float64, torch.float64]
    listed = outlier_statistic([T[0], T[1]], k=8, std_ratio=1.0, return_stats=True)
    for c in range(2):
        single = outlier_statistic(T[c], k=8, std_ratio=1.0, return_stats=True)
        want = outlier_numpy(neighbour_dist(P[c], 8), 8, 1.0)
        for b, l, s, w in zip(batch, listed, single, (want[2], want[0], want[1])):
            assert torch.equal(b[c], s) and torch.equal(l[c], s) and same(_np(s), w)
    assert torch.equal(outlier_statistic(T[0], k=8, std_ratio=1.0), batch[0][0])


def test_the_result_does_not_depend_on_the_search(gpu, monkeypatch):
    from parsenet_codebase_amd import kernels as K
    from parsenet_codebase_amd.cleaning import outlier_statistic
    T = torch.from_numpy(with_strays(3000, 8, strays=9)).to(gpu)
    brute, grid = (outlier_statistic(T, search=s, return_stats=True) for s in (None, "grid"))
    assert all(torch.equal(a, b) or (a.dtype == torch.float64 and same(_np(a), _np(b))) for a, b in zip(brute, grid))
    assert 2900 < int(brute[0].sum()) <= 2991
    calls = []
    real = K.knn3_grid
    monkeypatch.setattr(K, "knn3_grid", lambda *a, **kw: calls.append("grid") or real(*a, **kw))
    monkeypatch.setattr(K, "knn3_ragged", lambda *a, **kw: calls.append("brute"))
    big = torch.from_numpy(with_strays(12000, 9, strays=9)).to(gpu)
    keep = outlier_statistic(big, search="auto")
    assert calls == ["grid"] and 11000 < int(keep.sum()) <= 11991
    with pytest.raises(ValueError, match="search=\"grid\" lifts the limit"):
        outlier_statistic(big)


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
def test_degenerate_clouds_inside_a_batch(gpu, value):
    """A non-finite cloud ruins only itself; an empty cloud, one shorter than k and an all-coincident one."""
    from parsenet_codebase_amd.cleaning import outlier_statistic
    bad = with_strays(TILE + 50, 10)
    bad[TILE + 20, 1] = value
    clouds = [with_strays(500, 11), bad, np.zeros((0, 3), np.float32), with_strays(7, 12), identical(50),
              with_strays(1200, 13)]
    T = [torch.from_numpy(c).to(gpu) for c in clouds]
    for search in (None, "grid"):
        keep, a, stats = outlier_statistic(T, k=20, std_ratio=1.0, search=search, return_stats=True)
        for c, P in enumerate(clouds):
            want = outlier_numpy(neighbour_dist(P, 20), 20, 1.0)
            assert same(_np(a[c]), want[0]) and same(_np(stats[c]), want[1]) and same(_np(keep[c]), want[2]), (search, c)
        assert np.isnan(_np(a[1])).all() and np.isnan(_np(stats[1])).all() and not keep[1].any()
        assert np.isnan(_np(stats[2])[[0, 2]]).all() and _np(stats[2])[1] == 0
        assert (_np(a[3]) > 0).all() and (_np(a[4]) == 0).all() and not keep[4].any()
        assert int(keep[0].sum()) > 400 and int(keep[5].sum()) > 1000


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def torus_with_strays(n=100000, strays=200, seed=7):
    """The jittered torus (radius 0.95 about the origin) and ``strays`` points 2 .. 4 from the origin, shuffled
    -> (points, which are strays).  With k = 20 and std_ratio = 2 the numpy restatement removes the 200 strays and no
    torus point (checked on the CPU on fp64 KD-tree distances: mean 0.0165, std 0.0609, thr 0.138)."""
    rng = np.random.RandomState(seed)
    torus = _tool("orient_normals_ab").jittered_torus(n)[0]
    v = rng.normal(size=(strays, 3))
    v = (v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(2, 4, (strays, 1))).astype(np.float32)
    perm = rng.permutation(n + strays)
    return np.concatenate([torus, v])[perm], perm >= n


def test_a_hundred_thousand_points_with_strays_through_the_grid(gpu):
    from parsenet_codebase_amd import kernels as K
    from parsenet_codebase_amd.ragged import Clouds
    P, stray = torus_with_strays()
    clouds = Clouds(torch.from_numpy(P).to(gpu), "test")
    dist = K.knn3_grid(clouds.flat, clouds, None, 20, want_dist=True)[1]
    got = K.outlier_stat(dist, clouds, 20, 2.0)
    want = outlier_numpy(dist.cpu().numpy(), 20, 2.0)
    assert same(_np(got[0]), want[0]) and same(_np(got[1])[0], want[1]) and same(_np(got[2]), want[2])
    assert int(got[3][0]) == want[3] and same(_np(got[4]), want[4])
    keep = want[2].astype(bool)
    assert not keep[stray].any() and (~keep[~stray]).mean() <= 0.05


def test_remove_outliers_and_restore(gpu, monkeypatch):
    from parsenet_codebase_amd import _lib
    from parsenet_codebase_amd.cleaning import outlier_statistic, remove_outliers, restore
    reads = []
    real = _lib.pinned_like
    monkeypatch.setattr(_lib, "pinned_like", lambda shape, dtype, hold=False: (
        reads.append(tuple(shape)) if hold else None, real(shape, dtype, hold))[1])
    rng = np.random.RandomState(41)
    P = np.stack([with_strays(1300, 13, strays=20), with_strays(1300, 14, strays=5)])
    N = rng.normal(size=P.shape).astype(np.float32)
    L = rng.randint(0, 9, P.shape[:2])
    T, Nt, Lt = (torch.from_numpy(a).to(gpu) for a in (P, N, L))
    keep = outlier_statistic(T, std_ratio=1.0)
    assert reads == []                                          # no download in outlier_statistic
    pts, nrm, lab, index = remove_outliers(T, Nt, Lt, std_ratio=1.0)
    assert reads == [(2,)]                                      # one in remove_outliers: the kept counts
    assert all(isinstance(x, list) and len(x) == 2 for x in (pts, nrm, lab, index))
    for c in range(2):
        want = torch.nonzero(keep[c]).reshape(-1)
        assert index[c].dtype == torch.int64 and torch.equal(index[c], want) and 1000 < want.numel() < 1300
        assert torch.equal(pts[c], T[c][want]) and torch.equal(nrm[c], Nt[c][want]) and torch.equal(lab[c], Lt[c][want])
        back = restore(lab[c], index[c], 1300, -1)
        assert torch.equal(back, torch.where(keep[c], Lt[c], torch.full_like(Lt[c], -1)))
    assert all(torch.equal(a, b) for a, b in zip(restore(nrm, index, 1300, 0.0), [Nt[c] * keep[c][:, None] for c in (0, 1)]))
    # a single cloud comes back as tensors, a list as lists; the clouds may differ in size
    p1, n1, i1 = remove_outliers(T[0], Nt[0], std_ratio=1.0)
    assert torch.equal(p1, pts[0]) and torch.equal(n1, nrm[0]) and torch.equal(i1, index[0])
    pl, il = remove_outliers([T[0], T[1][:900]], std_ratio=1.0)
    assert torch.equal(pl[0], pts[0]) and torch.equal(il[0], index[0]) and pl[1].shape[0] == il[1].shape[0] <= 900
    assert len(reads) == 3
    # the errors
    with pytest.raises(ValueError, match="same layout"):
        remove_outliers(T, Nt[0])
    with pytest.raises(TypeError, match="float32"):
        remove_outliers(T.double())
    with pytest.raises(ValueError, match="outside the 5 points"):
        restore(lab[0][:2], torch.tensor([0, 5], device=gpu), 5, -1)


@pytest.mark.parametrize("seed", [101, 102, 103])
def test_against_the_fp64_oracle_outside_the_band_of_the_fp32_distances(gpu, seed):
    """oracle.ref_fitting.remove_outliers(P, 20, 0.5) on fp64 distances.  An fp32 distance carries at most 2.5 * 2^-24
    relative error (three squares, two sums, the root's argument halves it, one rounding to fp32), so a, mean, std and
    thr move by less than 1e-6 relative; the masks must agree wherever |a - thr| > 1e-5 thr, ten times that.  On the CPU
    the band holds no point of these clouds (500 .. 2 000 points; at most 0.5 % may lie in it)."""
    from oracle.ref_fitting import remove_outliers as oracle
    from parsenet_codebase_amd.cleaning import outlier_statistic
    rng = np.random.RandomState(seed)
    P = rng.uniform(-1, 1, (int(rng.randint(500, 2001)), 3)).astype(np.float32)
    n = P.shape[0]
    # the oracle's own statistic, restated to find its band; its mask is taken from what it returns
    Q = P.astype(np.float64)
    a = np.sort(np.sqrt(((Q[:, None, :] - Q[None, :, :]) ** 2).sum(2)), 1)[:, :20].mean(1)
    mean = a[a > 0].sum() / n
    thr = mean + 0.5 * np.sqrt(((a[a > 0] - mean) ** 2).sum() / (n - 1))
    kept = {tuple(row) for row in oracle(P, 20, 0.5).tolist()}
    mask = np.asarray([tuple(row) in kept for row in Q.tolist()])
    assert len(kept) == mask.sum() and np.array_equal(mask, (a > 0) & (a < thr))
    band = np.abs(a - thr) <= 1e-5 * thr
    assert band.sum() <= 0.005 * mask.sum()
    keep, ours, stats = outlier_statistic(torch.from_numpy(P).to(gpu), k=20, std_ratio=0.5, return_stats=True)
    assert np.array_equal(_np(keep).astype(bool)[~band], mask[~band])
    assert np.abs(_np(ours) - a).max() <= 1e-6 * a.max() and abs(_np(stats)[2] - thr) <= 1e-6 * thr


def purpose_cloud(seed=51):
    """A unit sphere of 20 000 points and 30 strays at 3 .. 10 radii, shuffled -> (points, which are strays)."""
    rng = np.random.RandomState(seed)
    v, w = rng.normal(size=(20000, 3)), rng.normal(size=(30, 3))
    sphere = v / np.linalg.norm(v, axis=1, keepdims=True)
    strays = w / np.linalg.norm(w, axis=1, keepdims=True) * rng.uniform(3, 10, (30, 1))
    perm = rng.permutation(20030)
    return np.concatenate([sphere, strays]).astype(np.float32)[perm], perm >= 20000


def covering_radius(X, C):
    """The largest distance from a point of X to its nearest point of C (float64: a judgement, not a bit pattern)."""
    d = ((X[:, None, :].astype(np.float64) - C[None, :, :].astype(np.float64)) ** 2).sum(-1)
    return float(np.sqrt(d.min(1).max()))


def test_farthest_point_sampling_stops_picking_strays(gpu):
    """On the CPU with the numpy restatements: 30 of the 64 raw samples are the strays, none after the removal, and the
    covering radius of the sphere drops from 0.491 to 0.334; the test asserts the inequalities only."""
    from parsenet_codebase_amd.cleaning import remove_outliers
    from parsenet_codebase_amd.sampling import farthest_point_sample
    P, stray = purpose_cloud()
    T = torch.from_numpy(P).to(gpu)
    raw = farthest_point_sample(T, 64).cpu().numpy()
    assert stray[raw].sum() == 30
    pts, index = remove_outliers(T, search="auto")
    index = index.cpu().numpy()
    assert not stray[index].any()
    clean = index[farthest_point_sample(pts, 64).cpu().numpy()]
    assert not stray[clean].any()
    before, after = covering_radius(P[~stray], P[raw]), covering_radius(P[~stray], P[clean])
    print("covering radius of the sphere: %.4f raw, %.4f after remove_outliers" % (before, after))
    assert after < before


def test_the_abi_on_the_gpu(gpu):
    from parsenet_codebase_amd import _lib
    lib = load_raw()
    k, n = 20, 2 * TILE + 9
    dist = neighbour_dist(with_strays(n, 15), k)
    D = torch.from_numpy(dist).to(gpu)
    off = torch.tensor([0, n], dtype=torch.int32, device=gpu)
    need = lib.pn_outlier_workspace_bytes(n, 1)
    ws = torch.zeros(need, dtype=torch.uint8, device=gpu)
    avg = torch.full((n,), -7.0, dtype=torch.float64, device=gpu)
    stats = torch.full((1, 3), -7.0, dtype=torch.float64, device=gpu)
    keep = torch.full((n,), 7, dtype=torch.uint8, device=gpu)
    kept = torch.full((1,), -7, dtype=torch.int32, device=gpu)
    real = dict(dist=D.data_ptr(), off=off.data_ptr(), S=1, total=n, k=k, std_ratio=2.0, avg=avg.data_ptr(),
                stats=stats.data_ptr(), keep=keep.data_ptr(), kept=kept.data_ptr(), ws=ws.data_ptr(), ws_bytes=need)
    check_invalid_arguments(lib, **real)                        # a workspace one byte short among them
    torch.cuda.synchronize()
    assert (avg == -7).all() and (stats == -7).all() and (keep == 7).all() and (kept == -7).all() and (ws == 0).all()
    assert raw_call(lib, **dict(real, index=None, stream=_lib.current_stream(gpu))) == 0      # index = NULL
    torch.cuda.synchronize()
    want = outlier_numpy(dist, k, 2.0)
    assert same(avg.cpu().numpy(), want[0]) and same(stats.cpu().numpy()[0], want[1])
    assert same(keep.cpu().numpy(), want[2]) and int(kept[0]) == want[3]
