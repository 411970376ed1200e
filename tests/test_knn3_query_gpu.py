"""GPU checks of the cross-cloud neighbour query (csrc/knn3_query.hip) and the k-NN lifting on it (csrc/knn_lift.hip,
parsenet_codebase_amd/neighbors.py): the adversarial inputs of tests/test_knn3_query_abi.py at full size against the
numpy brute force in the same fp32 arithmetic, the self-query against knn3_grid, k = 1 against chamfer_nn_ragged,
independence of the batching, the non-finite rules, both lifting rules against their restatements, lift_knn at k = 1
against lift, and the Python contract.  Every comparison is exact: there is no tolerance in this file."""
import numpy as np
import pytest
import torch

from tests.test_knn3_grid_abi import tight_pairs
from tests.test_knn3_query_abi import (adversarial, brute, interpolate_ref, outside_queries, same_bits, unit_box,
                                       vote_ref)

pytestmark = pytest.mark.gpu


def _off(sizes, gpu):
    return torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)).to(gpu)


def _flat(clouds, gpu):
    return torch.from_numpy(np.concatenate([np.asarray(c, np.float32).reshape(-1, 3) for c in clouds])).to(gpu)


def _query(gpu, refs, qrys, k):
    """knn3_query on a ragged batch of numpy (reference, query) pairs -> (idx, dist) as numpy."""
    from parsenet_codebase_amd import kernels as K
    idx, dist = K.knn3_query(_flat(refs, gpu), _off([len(r) for r in refs], gpu), _flat(qrys, gpu),
                             _off([len(q) for q in qrys], gpu), k, want_dist=True)
    return idx.cpu().numpy(), dist.cpu().numpy()


def _check(gpu, refs, qrys, k, what):
    """The query of a batch against the brute force of every pair: idx exactly, dist bit for bit."""
    idx, dist = _query(gpu, refs, qrys, k)
    o = 0
    for R, Q in zip(refs, qrys):
        want_idx, want_dist = brute(R, Q, k)
        got = idx[o:o + len(Q)]
        assert np.array_equal(got, want_idx), (what, len(R), len(Q), k, int((got != want_idx).any(1).sum()))
        assert same_bits(dist[o:o + len(Q)], want_dist), (what, len(R), len(Q), k)
        o += len(Q)
    return idx, dist


@pytest.mark.parametrize("name", sorted(adversarial(4)))
def test_adversarial_inputs_at_full_size(gpu, name):
    R, Q, ks = adversarial(4)[name]
    for k in ks:
        _check(gpu, [R], [Q], k, name)


def test_large_against_small_both_ways(gpu):
    """12 000 reference points x 3 000 queries and 300 x 12 000, in one ragged batch; a third of the queries outside."""
    rng = np.random.RandomState(70)
    big, small = tight_pairs(12000, 5), rng.uniform(-0.5, 0.5, (300, 3)).astype(np.float32)
    q1 = np.concatenate([rng.uniform(-0.5, 0.5, (2000, 3)), rng.uniform(-3, 3, (1000, 3))]).astype(np.float32)
    q2 = np.concatenate([tight_pairs(8000, 6), rng.uniform(-3, 3, (4000, 3)).astype(np.float32)])
    _check(gpu, [big, small], [q1, q2], 16, "(12000 x 3000, 300 x 12000)")


@pytest.mark.parametrize("k", [1, 5, 16, 64])
def test_the_self_query_equals_knn3_grid(gpu, k):
    from parsenet_codebase_amd import kernels as K
    sizes = [64, 700, 2600, 9000]
    flat = torch.from_numpy(np.concatenate([tight_pairs(n, 3 + k + n) for n in sizes])).to(gpu)
    off = _off(sizes, gpu)
    want_idx, want_dist = K.knn3_grid(flat, off, max(sizes), k, want_dist=True)
    idx, dist = K.knn3_query(flat, off, flat, off, k, want_dist=True)
    assert torch.equal(idx, want_idx), int((idx != want_idx).any(1).sum())
    assert torch.equal(dist.view(torch.int32), want_dist.view(torch.int32))
    assert torch.equal(K.knn3_query(flat, off, flat, off, k), want_idx)                       # without the distances


def test_a_segment_shorter_than_k_differs_from_knn3_grid_exactly_in_the_padding(gpu):
    from parsenet_codebase_amd import kernels as K
    sizes, k = [5, 300], 8
    flat = torch.from_numpy(np.concatenate([tight_pairs(n, 9 + n) for n in sizes])).to(gpu)
    off = _off(sizes, gpu)
    gi, gd = K.knn3_grid(flat, off, max(sizes), k, want_dist=True)
    qi, qd = K.knn3_query(flat, off, flat, off, k, want_dist=True)
    assert torch.equal(qi[5:], gi[5:]) and torch.equal(qd[5:].view(torch.int32), gd[5:].view(torch.int32))
    assert torch.equal(qi[:5, :5], gi[:5, :5]) and torch.equal(qd[:5, :5].view(torch.int32), gd[:5, :5].view(torch.int32))
    assert (qi[:5, 5:] == -1).all() and torch.isinf(qd[:5, 5:]).all() and (qd[:5, 5:] > 0).all()          # -1 / +inf here
    assert torch.equal(gi[:5, 5:], torch.arange(5, device=gpu, dtype=torch.int32)[:, None].expand(5, 3))  # itself there
    assert (gd[:5, 5:] == 0).all()


def test_k1_against_the_brute_force_chamfer_kernel(gpu):
    """argA equal, dist == (float) sqrt((double) minA) bit for bit, on items of very different size.  The batch of the
    query also holds an item with an EMPTY reference; chamfer_nn_ragged's contract excludes empty items (chamfer.hip:
    "Items must be non-empty"), so it gets the other items, and the empty item is held to its definition."""
    from parsenet_codebase_amd import kernels as K
    rng = np.random.RandomState(71)
    na, nb = [3000, 17, 5000, 900], [40, 6000, 2500, 1]
    A = [rng.uniform(-1, 1, (n, 3)).astype(np.float32) for n in na]
    Bc = [rng.uniform(-1, 1, (n, 3)).astype(np.float32) for n in nb]
    minA, argA, _, _ = K.chamfer_nn_ragged(_flat(A, gpu), _off(na, gpu), max(na), _flat(Bc, gpu), _off(nb, gpu), max(nb),
                                           side_b=False)
    extra = rng.uniform(-1, 1, (33, 3)).astype(np.float32)
    qa, qb = A[:2] + [extra] + A[2:], Bc[:2] + [np.zeros((0, 3), np.float32)] + Bc[2:]
    idx, dist = K.knn3_query(_flat(qb, gpu), _off([len(b) for b in qb], gpu), _flat(qa, gpu),
                             _off([len(a) for a in qa], gpu), 1, want_dist=True)
    lo = sum(na[:2])
    keep = np.r_[0:lo, lo + 33:lo + 33 + sum(na[2:])]
    assert (idx[lo:lo + 33] == -1).all() and (dist[lo:lo + 33] == float("inf")).all()
    assert np.array_equal(idx.cpu().numpy()[keep, 0], argA.cpu().numpy())
    want = np.sqrt(minA.cpu().numpy().astype(np.float64)).astype(np.float32)
    assert same_bits(dist.cpu().numpy()[keep, 0], want)


def test_every_batching_gives_the_same_bits(gpu):
    empty = np.zeros((0, 3), np.float32)
    refs = [unit_box(500, 73), empty, unit_box(3000, 74), unit_box(40, 75), empty, unit_box(2, 76)]
    qrys = [outside_queries(4, 77), unit_box(30, 78), empty, unit_box(700, 79), empty, unit_box(90, 80)]
    k = 5
    idx, dist = _check(gpu, refs, qrys, k, "ragged with empty segments")
    again = _query(gpu, refs, qrys, k)
    assert np.array_equal(again[0], idx) and same_bits(again[1], dist)                        # run to run
    o = 0
    for R, Q in zip(refs, qrys):
        if len(Q):
            one = _query(gpu, [R], [Q], k)
            assert np.array_equal(one[0], idx[o:o + len(Q)]) and same_bits(one[1], dist[o:o + len(Q)])
        o += len(Q)


def test_non_finite_rows(gpu):
    refs = [unit_box(400, 81), unit_box(300, 82), unit_box(200, 83)]
    qrys = [unit_box(100, 84), unit_box(150, 85), unit_box(50, 86)]
    want = _query(gpu, refs, qrys, 4)
    q = [x.copy() for x in qrys]
    q[1][7, 2] = np.nan                                      # one NaN query: that row only
    idx, dist = _query(gpu, refs, q, 4)
    row = 100 + 7
    assert (idx[row] == -1).all() and np.isnan(dist[row]).all()
    assert np.array_equal(np.delete(idx, row, 0), np.delete(want[0], row, 0))
    assert same_bits(np.delete(dist, row, 0), np.delete(want[1], row, 0))
    r = [x.copy() for x in refs]
    r[1][250, 0] = np.inf                                    # one inf reference point: all rows of that segment only
    idx, dist = _query(gpu, r, qrys, 4)
    assert (idx[100:250] == -1).all() and np.isnan(dist[100:250]).all()
    rest = np.r_[0:100, 250:300]
    assert np.array_equal(idx[rest], want[0][rest]) and same_bits(dist[rest], want[1][rest])


# ---------------------------------------------------------------------------------------------
# lifting
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lift_case():
    """(samples per cloud, points per cloud): the second cloud has two samples (n_r < k for k = 3, 8), and points
    coincident with samples."""
    s = [unit_box(500, 90), unit_box(2, 91)]
    p = [np.concatenate([s[0][:40], unit_box(1200, 92), outside_queries(1, 93)]), np.concatenate([s[1], unit_box(70, 94)])]
    return s, p


@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("C", [1, 3, 50])
def test_lift_knn_interpolates_as_the_fp64_restatement(gpu, lift_case, C, k):
    from parsenet_codebase_amd import neighbors
    s, p = lift_case
    rng = np.random.RandomState(95 + C + k)
    values = [rng.normal(0, 10, (len(x), C) if C > 1 else (len(x),)).astype(np.float32) for x in s]
    out = neighbors.lift_knn([torch.from_numpy(v).to(gpu) for v in values], [torch.from_numpy(x).to(gpu) for x in p],
                             [torch.from_numpy(x).to(gpu) for x in s], k=k)
    for b in range(2):
        idx, dist = brute(s[b], p[b], k)
        want = interpolate_ref(values[b].reshape(len(s[b]), C), idx, dist).reshape((len(p[b]),) + values[b].shape[1:])
        assert same_bits(out[b].cpu().numpy(), want), (b, C, k)
    if k == 1:                                               # a point coincident with a sample takes its row exactly
        assert np.array_equal(out[0].cpu().numpy()[:40], values[0][:40])


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_lift_knn_votes_as_the_python_restatement(gpu, lift_case, dtype):
    from parsenet_codebase_amd import neighbors
    s, p = lift_case
    rng = np.random.RandomState(96)
    for k in (1, 3, 4, 8):                                   # an even k: ties between two labels
        labels = [rng.randint(-1, 3, len(x)).astype(np.int32) for x in s]
        out = neighbors.lift_knn([torch.from_numpy(v).to(gpu).to(dtype) for v in labels],
                                 [torch.from_numpy(x).to(gpu) for x in p], [torch.from_numpy(x).to(gpu) for x in s], k=k)
        for b in range(2):
            assert out[b].dtype == dtype
            assert np.array_equal(out[b].cpu().numpy(), vote_ref(labels[b], brute(s[b], p[b], k)[0])), (b, k)


def test_lift_knn_with_one_neighbour_equals_lift_by_owner(gpu):
    """lift_knn(v, points, points[sample], k=1) == lift(v, owner) with owner from reduce_cloud.  The cloud holds no
    duplicate points: FPS breaks ties by rank, the query by reference index, and these agree only when distinct
    samples are distinct points."""
    from parsenet_codebase_amd import neighbors, sampling
    P = np.random.RandomState(97).uniform(-1, 1, (2, 5000, 3)).astype(np.float32)
    assert all(len(np.unique(c, axis=0)) == len(c) for c in P)
    pts = torch.from_numpy(P).to(gpu)
    reduced, owner = sampling.reduce_cloud(pts, 257)
    g = torch.Generator().manual_seed(1)
    rows = torch.randn(2, 257, 6, generator=g).to(gpu)
    labels = torch.randint(0, 9, (2, 257), generator=g).to(gpu)
    assert torch.equal(neighbors.lift_knn(rows, pts, reduced, k=1), sampling.lift(rows, owner))
    assert torch.equal(neighbors.lift_knn(labels, pts, reduced, k=1), sampling.lift(labels, owner))
    idx = neighbors.nearest(pts, reduced)
    assert idx.dtype == torch.int64 and torch.equal(idx[..., 0], owner)
    d = neighbors.cloud_distance(pts, reduced)
    assert d.shape == (2, 5000) and torch.equal(d, neighbors.nearest(pts, reduced, return_dist=True)[1][..., 0])


def test_the_python_contract(gpu):
    from parsenet_codebase_amd import neighbors
    a, b = torch.zeros(8, 3, device=gpu), torch.ones(5, 3, device=gpu)
    with pytest.raises(ValueError, match="2 clouds of points against 1"):
        neighbors.nearest([a, a], [b])
    with pytest.raises(ValueError, match="clouds"):
        neighbors.lift_knn(torch.zeros(5, device=gpu), torch.zeros(2, 8, 3, device=gpu), b)
    with pytest.raises(TypeError, match="float32"):
        neighbors.nearest(a.double(), b)
    with pytest.raises(TypeError, match="float32"):
        neighbors.cloud_distance(a, b.half())
    with pytest.raises(TypeError, match="float32 .* or int32 / int64"):
        neighbors.lift_knn(torch.zeros(5, device=gpu, dtype=torch.float64), a, b)
    with pytest.raises(TypeError, match="float32 .* or int32 / int64"):
        neighbors.lift_knn(torch.zeros(5, device=gpu, dtype=torch.bool), a, b)
    with pytest.raises(ValueError, match="same layout and sizes"):
        neighbors.lift_knn(torch.zeros(4, device=gpu), a, b)
    with pytest.raises(RuntimeError, match="MI355X only"):
        neighbors.nearest(a.cpu(), b)
    with pytest.raises(RuntimeError, match="MI355X only"):
        neighbors.lift_knn(torch.zeros(5), a, b)
    for k in (0, 65, -1):
        with pytest.raises(ValueError, match="k must be 1 .. 64"):
            neighbors.nearest(a, b, k=k)
        with pytest.raises(ValueError, match="k must be 1 .. 64"):
            neighbors.lift_knn(torch.zeros(5, device=gpu), a, b, k=k)
    with pytest.raises(TypeError, match="k must be an integer"):
        neighbors.nearest(a, b, k=2.0)
    idx, dist = neighbors.nearest(a, b, k=7, return_dist=True)              # n_r = 5 < k
    assert idx.shape == (8, 7) and (idx[:, 5:] == -1).all() and torch.isinf(dist[:, 5:]).all()
    assert neighbors.cloud_distance(torch.zeros(2, 8, 3, device=gpu), [b, b]).shape == (2, 8)
