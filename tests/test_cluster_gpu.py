"""GPU checks of the Euclidean cluster extraction (csrc/cluster.hip, parsenet_codebase_amd/cleaning.py): label, ncomp,
count, first and ndrop equal to the numpy restatement of the definition (tests.test_cluster_abi.cluster_numpy) on the
clouds and the ragged batch of the CPU tests, on a second run, alone and in a batch, and on one cloud of 30 000 points;
euclidean_clusters, split_clusters and keep_largest in their three layouts, with gathered per-point arrays, their one
host read and their errors.  Every comparison is exact: there is no tolerance in this file."""
import numpy as np
import pytest
import torch

from tests.test_cluster_abi import (BAD_RADII, cases, check_properties, cluster_numpy, cluster_numpy_batch, equal,
                                    ragged_batch, same, torus, uniform)

pytestmark = pytest.mark.gpu
OUTPUTS = ("label", "ncomp", "count", "first", "ndrop")


def _off(sizes, gpu):
    return torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)).to(gpu)


def _cluster(gpu, clouds, radii, min_size=1, as_clouds=False):
    """kernels.cluster_ragged on a ragged batch of numpy clouds -> (label, ncomp, count, first, ndrop) as numpy."""
    from parsenet_codebase_amd import kernels as K
    from parsenet_codebase_amd.ragged import Clouds
    rad = torch.from_numpy(np.asarray(radii, np.float32)).to(gpu)
    if as_clouds:
        off = Clouds([torch.from_numpy(np.ascontiguousarray(c, np.float32).reshape(-1, 3)).to(gpu) for c in clouds], "test")
        flat = off.flat
    else:
        flat = torch.from_numpy(np.concatenate([c.reshape(-1, 3) for c in clouds]).astype(np.float32)).to(gpu)
        off = _off([c.shape[0] for c in clouds], gpu)
    return tuple(o.cpu().numpy() for o in K.cluster_ragged(flat, off, rad, min_size))


def _check(gpu, clouds, radii, min_size=1, what="", want=None):
    got = _cluster(gpu, clouds, radii, min_size)
    want = cluster_numpy_batch(clouds, radii, min_size) if want is None else want
    for name, g, w in zip(OUTPUTS, got, want):
        assert same(g, np.asarray(w, g.dtype)), "%s: %s differs" % (what, name)
    again = _cluster(gpu, clouds, radii, min_size, as_clouds=True)      # a second run, the schedule of the largest cloud
    assert all(same(a, b) for a, b in zip(got, again)), "%s: a second run changed a result" % what
    return got


@pytest.fixture(scope="module")
def reference():
    """name -> cluster_numpy of the case: computed once, shared, never changed."""
    return {name: cluster_numpy(*case) for name, case in cases().items()}


@pytest.mark.parametrize("name", sorted(cases()))
def test_the_kernels_equal_the_definition(gpu, reference, name):
    P, r, min_size = cases()[name]
    w = reference[name]
    got = _check(gpu, [P], [r], min_size, name, want=(w[0], [w[1]], w[2], w[3], [w[4]]))
    check_properties(P, (got[0], int(got[1][0]), got[2], got[3], int(got[4][0])))


def test_the_ragged_batch_alone_and_in_the_batch(gpu):
    clouds, radii = ragged_batch()
    for min_size in (1, 3):
        got = _check(gpu, clouds, radii, min_size, "ragged batch")
        assert got[1].tolist()[1:4] == [0, 1 if min_size == 1 else 0, -1] and got[1][5] == -1 and got[1][7] == -2
        o = 0
        for c, P in enumerate(clouds):
            alone = _cluster(gpu, [P], [radii[c]], min_size)
            n = P.shape[0]
            assert alone[1][0] == got[1][c] and alone[4][0] == got[4][c]
            assert equal([alone[t] for t in (0, 2, 3)], [got[t][o:o + n] for t in (0, 2, 3)])
            o += n
    # another batching of the same clouds, another order
    order = [6, 3, 0, 1, 7, 2, 5, 4]
    got = _check(gpu, [clouds[c] for c in order], [radii[c] for c in order], 1, "ragged batch, reordered")
    empty = clouds[1]
    _check(gpu, [empty, empty], [0.5, 0.0], 1, "empty clouds only")
    _check(gpu, [empty, clouds[4], empty, empty], [0.5, 0.9, 0.3, 0.2], 1, "empty clouds around one")


def test_statuses(gpu):
    P = uniform(65)
    Q = P.copy()
    Q[7, 2] = np.inf
    for bad in BAD_RADII:
        got = _check(gpu, [P, Q, P], [bad, bad, 0.4], 1, "radius = %r" % bad)
        assert got[1].tolist()[:2] == [-2, -1] and got[1][2] >= 1 and (got[0][:130] == -1).all()


def scene_30000():
    """Five jittered tori of 6 000 points, 4 apart; the radius three times the mean spacing."""
    P = np.concatenate([torus(6000, 50 + t, centre=(4.0 * t, 0.3 * t, 0), jitter=0.005) for t in range(5)])
    spacing = np.sqrt(4 * np.pi ** 2 * 1.0 * 0.3 / 6000)
    return P[np.random.RandomState(55).permutation(P.shape[0])].astype(np.float32), float(3 * spacing)


def test_one_cloud_of_30000_points(gpu):
    """Above the 10 240 points of the one-workgroup kernels; the restatement block-wise, 1 024 rows against all."""
    P, r = scene_30000()
    want = cluster_numpy(P, r, 10)
    assert want[1] == 5 and (want[2][:5] == 6000).all()
    got = _check(gpu, [P], [r], 10, "30 000 points", want=(want[0], [want[1]], want[2], want[3], [want[4]]))
    check_properties(P, (got[0], int(got[1][0]), got[2], got[3], int(got[4][0])))


def test_want_selects_the_outputs(gpu):
    from parsenet_codebase_amd import kernels as K
    P, r, _ = cases()["torus and a clump"]
    T, rad = torch.from_numpy(P).to(gpu), torch.tensor([r], device=gpu)
    off = _off([P.shape[0]], gpu)
    full = K.cluster_ragged(T, off, rad, 1)
    assert len(full) == 5 and len(K.cluster_ragged(T, off, rad, 1, want=())) == 2
    some = K.cluster_ragged(T, off, rad, 1, want=("ndrop", "count"))
    assert len(some) == 4 and torch.equal(some[2], full[2]) and torch.equal(some[3], full[4])
    with pytest.raises(ValueError, match="want holds"):
        K.cluster_ragged(T, off, rad, 1, want=("rep",))
    with pytest.raises(ValueError, match="min_size must be"):
        K.cluster_ragged(T, off, rad, 0)
    with pytest.raises(ValueError, match="radius must be"):
        K.cluster_ragged(T, off, torch.ones(2, device=gpu), 1)


# ---------------------------------------------------------------------------------------------
# cleaning.py
# ---------------------------------------------------------------------------------------------
def scene(seed, n0=700, n1=500, clump=30):
    """Two tori and a clump of stray points, shuffled; radius 0.39 is three spacings of the sparser torus."""
    rng = np.random.RandomState(seed)
    P = np.concatenate([torus(n0, seed), torus(n1, seed + 1, centre=(4.0, 0, 0)),
                        0.01 * rng.uniform(-1, 1, (clump, 3)) + np.asarray([2.0, 3.0, 0.0])]).astype(np.float32)
    return P[rng.permutation(P.shape[0])]


RADIUS = 0.39


def _count_reads(monkeypatch):
    from parsenet_codebase_amd import _lib
    reads = []
    real = _lib.pinned_like
    monkeypatch.setattr(_lib, "pinned_like", lambda shape, dtype, hold=False: (
        reads.append(tuple(shape)) if hold else None, real(shape, dtype, hold))[1])
    return reads


def _check_split(P, N, parts, want, order="index"):
    """The components of one cloud against the restatement."""
    label, C, count = want[0], want[1], want[2]
    ranks = list(range(C)) if order == "index" else sorted(range(C), key=lambda c: (-int(count[c]), c))
    assert len(parts) == C
    for (pts, nrm, index), c in zip(parts, ranks):
        rows = np.flatnonzero(label == c)
        assert index.dtype == torch.int64 and np.array_equal(index.cpu().numpy(), rows)
        assert same(pts.cpu().numpy(), P[rows]) and same(nrm.cpu().numpy(), N[rows])


def test_split_clusters_single_cloud_and_restore(gpu, monkeypatch):
    from parsenet_codebase_amd.cleaning import euclidean_clusters, restore, split_clusters
    reads = _count_reads(monkeypatch)
    P = scene(61)
    n = P.shape[0]
    N = np.random.RandomState(62).normal(size=P.shape).astype(np.float32)
    T, Nt = torch.from_numpy(P).to(gpu), torch.from_numpy(N).to(gpu)
    want = cluster_numpy(P, RADIUS)
    assert want[1] == 3 and sorted(want[2][:3].tolist()) == [30, 500, 700]
    label, ncomp, count, first = euclidean_clusters(T, RADIUS, return_info=True)
    assert reads == []                                          # no download in euclidean_clusters
    assert label.dtype == torch.int32 and same(label.cpu().numpy(), want[0]) and int(ncomp) == 3
    assert same(count.cpu().numpy(), want[2]) and same(first.cpu().numpy(), want[3])
    assert torch.equal(euclidean_clusters(T, RADIUS), label)
    parts = split_clusters(T, Nt, radius=RADIUS)
    assert reads == [(1 + n,)]                                  # one in split_clusters: ncomp and the sizes
    _check_split(P, N, parts, want)
    back = restore(torch.cat([p[0] for p in parts]), torch.cat([p[2] for p in parts]), n, float("nan"))
    assert torch.equal(back, T)                                 # restore over the indices reassembles the scan
    _check_split(P, N, split_clusters(T, Nt, radius=RADIUS, order="size"), want, "size")
    sized = [p[0].shape[0] for p in split_clusters(T, Nt, radius=RADIUS, order="size")]
    assert sized == [700, 500, 30]
    big = cluster_numpy(P, RADIUS, 31)
    parts = split_clusters(T, Nt, radius=RADIUS, min_size=31)
    _check_split(P, N, parts, big)
    assert len(parts) == 2 and same(euclidean_clusters(T, RADIUS, min_size=31).cpu().numpy(), big[0])
    lab = restore([torch.full((p[2].shape[0],), c, device=gpu) for c, p in enumerate(parts)], [p[2] for p in parts], n, -1)
    assert same(torch.stack(lab).max(0).values.cpu().numpy().astype(np.int32), big[0])      # the clump stays -1


def test_the_three_functions_on_a_batch_and_a_list(gpu, monkeypatch):
    from parsenet_codebase_amd.cleaning import euclidean_clusters, keep_largest, split_clusters
    reads = _count_reads(monkeypatch)
    rng = np.random.RandomState(63)
    # a batch (B,N,3)
    B = np.stack([scene(64), scene(65)])
    NB = rng.normal(size=B.shape).astype(np.float32)
    T, Nt = torch.from_numpy(B).to(gpu), torch.from_numpy(NB).to(gpu)
    want = [cluster_numpy(B[c], RADIUS) for c in range(2)]
    label, ncomp, count, first = euclidean_clusters(T, RADIUS, return_info=True)
    assert tuple(label.shape) == (2, 1230) and ncomp.tolist() == [w[1] for w in want]
    for c in range(2):
        assert same(label[c].cpu().numpy(), want[c][0]) and same(count[c].cpu().numpy(), want[c][2])
        assert same(first[c].cpu().numpy(), want[c][3])
    parts = split_clusters(T, Nt, radius=RADIUS)
    assert reads == [(2 + 2 * 1230,)] and isinstance(parts, list) and len(parts) == 2
    for c in range(2):
        _check_split(B[c], NB[c], parts[c], want[c])
    pts, nrm, index = keep_largest(T, Nt, radius=RADIUS)
    assert all(isinstance(x, list) and len(x) == 2 for x in (pts, nrm, index)) and len(reads) == 2
    for c in range(2):
        rows = np.flatnonzero(want[c][0] == int(np.argmax(want[c][2])))
        assert rows.size == 700 and np.array_equal(index[c].cpu().numpy(), rows)
        assert same(pts[c].cpu().numpy(), B[c][rows]) and same(nrm[c].cpu().numpy(), NB[c][rows])
    # a list: different sizes, a radius per cloud, an empty cloud and a non-finite one
    bad = scene(66, 200, 100, 5)
    bad[17, 0] = np.nan
    L = [scene(67, 400, 300, 10), np.zeros((0, 3), np.float32), bad, scene(68, 300, 300, 40)]
    radii = [0.5, 0.3, 0.4, 0.55]
    NL = [rng.normal(size=c.shape).astype(np.float32) for c in L]
    TL, NtL = [torch.from_numpy(c).to(gpu) for c in L], [torch.from_numpy(c).to(gpu) for c in NL]
    want = [cluster_numpy(c, r) for c, r in zip(L, radii)]
    assert [w[1] for w in want] == [3, 0, -1, 3]
    label, ncomp, count, first = euclidean_clusters(TL, radii, return_info=True)
    assert [int(v) for v in ncomp] == [3, 0, -1, 3]
    for c in range(4):
        assert same(label[c].cpu().numpy(), want[c][0]) and same(first[c].cpu().numpy(), want[c][3])
    for order in ("index", "size"):
        parts = split_clusters(TL, NtL, radius=radii, order=order)
        assert len(parts) == 4 and parts[1] == [] and parts[2] == []      # empty; non-finite: no component
        for c in (0, 3):
            _check_split(L[c], NL[c], parts[c], want[c], order)
    pts, nrm, index = keep_largest(TL, NtL, radius=radii)
    assert [p.shape[0] for p in pts] == [400, 0, 0, 300] and index[1].dtype == torch.int64
    assert tuple(nrm[2].shape) == (0, 3)
    rows = np.flatnonzero(want[3][0] == int(np.argmax(want[3][2])))         # two components of 300: the lower index wins
    assert np.array_equal(index[3].cpu().numpy(), rows) and sorted(want[3][2][:3].tolist()) == [40, 300, 300]
    with pytest.raises(ValueError, match="cloud 1"):                         # status -2: the square underflows
        split_clusters([TL[0], TL[3]], radius=[0.5, 1e-30])
    assert [int(v) for v in euclidean_clusters([TL[0], TL[3]], [0.5, 1e-30], return_info=True)[1]] == [3, -2]


def test_keep_largest_drops_the_clump_the_statistic_keeps(gpu):
    """The case this feature exists for: a clump of thirty stray points has small neighbour distances."""
    from parsenet_codebase_amd.cleaning import keep_largest, outlier_statistic, restore
    P, r, _ = cases()["torus and a clump"]                      # 900 points of a torus, then the clump
    T = torch.from_numpy(P).to(gpu)
    colour = torch.arange(930, device=gpu)
    pts, col, index = keep_largest(T, colour, radius=r)
    assert np.array_equal(index.cpu().numpy(), np.arange(900)) and torch.equal(pts, T[:900])
    assert torch.equal(col, colour[:900])
    assert restore(col, index, 930, -1)[900:].eq(-1).all()
    keep = outlier_statistic(T)
    assert keep[900:].any()                                     # the statistical filter keeps part of the clump


def test_bad_arguments_raise_before_any_gpu_call(gpu, monkeypatch):
    from parsenet_codebase_amd import cleaning
    from parsenet_codebase_amd import kernels as K

    def never(*a, **k):
        raise AssertionError("the GPU was called")
    monkeypatch.setattr(K, "cluster_ragged", never)
    T = torch.zeros(8, 3, device=gpu)
    for fn in (cleaning.euclidean_clusters, cleaning.split_clusters, cleaning.keep_largest):
        for radius in (0, -1.0, float("nan"), float("inf"), None, [0.1, 0.2]):
            with pytest.raises(ValueError, match="radius"):
                fn(T, radius=radius)
    for fn in (cleaning.euclidean_clusters, cleaning.split_clusters):
        for min_size in (0, 1.5, True):
            with pytest.raises(ValueError, match="min_size must be"):
                fn(T, radius=0.1, min_size=min_size)
    with pytest.raises(ValueError, match="order must be"):
        cleaning.split_clusters(T, radius=0.1, order="largest")
