"""GPU checks of the uniform-grid neighbour search (csrc/knn3_grid.hip): idx and dist bit-identical to the brute-force
kernel (knn3_ragged) wherever both run, equal to a block-wise numpy brute force in the same arithmetic above its limit,
the adversarial inputs of tests/test_knn3_grid_abi.py at full size, independence of the batching, and the argument
contract.  Every comparison is exact: there is no tolerance in this file."""
import numpy as np
import pytest
import torch

from tests.test_knn3_grid_abi import (adversarial, check_invalid_arguments, load_raw, tight_pairs)

pytestmark = pytest.mark.gpu


def brute(P, k, rows=1000):
    """(idx (n,k) int32, d (n,k) fp32) by knn3's rule, 1 000 query rows at a time: d = ((dx^2 + dy^2) + dz^2) in fp32,
    ordered by (d, j), a cloud of fewer than k points padded with the point itself.  The order is np.lexsort's on
    (j, d).  A full lexsort of 12 000 x 12 000 values takes half a minute, so it is taken in two steps: np.partition
    gives every row's k-th smallest d, and the lexsort runs over the candidates with d <= that value only — every
    tie at the k-th value among them.  The literal lexsort of whole rows is run on a sample of rows in
    test_above_the_limit_of_the_brute_force_kernel."""
    P = np.ascontiguousarray(P, np.float32)
    n = P.shape[0]
    kk = min(k, n)
    idx, dd = np.empty((n, k), np.int32), np.zeros((n, k), np.float32)
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    for a in range(0, n, rows):
        dx, dy, dz = x[a:a + rows, None] - x[None, :], y[a:a + rows, None] - y[None, :], z[a:a + rows, None] - z[None, :]
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
        dd[a:a + rows, :kk] = d[take]
    idx[:, kk:] = np.arange(n)[:, None]
    return idx, dd


def _off(sizes, gpu):
    return torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)).to(gpu)


def _grid(gpu, clouds, k):
    """knn3_grid on a ragged batch of numpy clouds -> (idx, dist) as numpy."""
    from parsenet_codebase_amd import kernels as K
    sizes = [c.shape[0] for c in clouds]
    flat = torch.from_numpy(np.concatenate(clouds).astype(np.float32).reshape(-1, 3)).to(gpu)
    idx, dist = K.knn3_grid(flat, _off(sizes, gpu), max(max(sizes), 1), k, want_dist=True)
    return idx.cpu().numpy(), dist.cpu().numpy()


def _check(gpu, clouds, k, what):
    """The grid search of a batch against the block-wise brute force of every cloud: idx exactly, dist bit for bit."""
    idx, dist = _grid(gpu, clouds, k)
    o = 0
    for c in clouds:
        n = c.shape[0]
        want, d2 = brute(c, k)
        got = idx[o:o + n]
        assert np.array_equal(got, want), (what, n, k, int((got != want).any(1).sum()))
        assert np.array_equal(dist[o:o + n].view(np.uint32), np.sqrt(d2.astype(np.float64)).astype(np.float32).view(np.uint32)), (what, n, k)
        o += n
    return idx, dist


@pytest.mark.parametrize("k", [1, 5, 16, 64])
def test_bit_identical_to_the_brute_force_kernel_on_a_ragged_batch(gpu, k):
    from parsenet_codebase_amd import kernels as K
    sizes = [1, 7, 64, 700, 2600, 9000]
    flat = torch.from_numpy(np.concatenate([tight_pairs(n, 3 + k + n) for n in sizes])).to(gpu)
    off = _off(sizes, gpu)
    want_idx, want_dist = K.knn3_ragged(flat, off, max(sizes), k, want_dist=True)
    idx, dist = K.knn3_grid(flat, off, max(sizes), k, want_dist=True)
    assert torch.equal(idx, want_idx), int((idx != want_idx).any(1).sum())
    assert torch.equal(dist, want_dist) and torch.equal(dist.view(torch.int32), want_dist.view(torch.int32))     # +0 too
    assert torch.equal(K.knn3_grid(flat, off, max(sizes), k), want_idx)                       # without the distances
    again = K.knn3_grid(flat, off, max(sizes), k, want_dist=True)
    assert torch.equal(again[0], idx) and torch.equal(again[1], dist)                         # run to run


def test_above_the_limit_of_the_brute_force_kernel(gpu):
    rng = np.random.RandomState(21)
    big, small = tight_pairs(12000, 5), rng.uniform(-0.5, 0.5, (300, 3)).astype(np.float32)
    idx, dist = _check(gpu, [big, small], 16, "ragged (12000, 300)")
    rows = np.r_[0:100, 5950:6050, 11900:12000]                       # the literal np.lexsort on 300 query rows
    d = big[rows, None, :] - big[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    assert np.array_equal(np.lexsort((np.broadcast_to(np.arange(12000), d2.shape), d2), axis=1)[:, :16], idx[rows])
    alone = _grid(gpu, [big], 16)                                     # one cloud of 12 000 points: the same bits
    assert np.array_equal(alone[0], idx[:12000]) and np.array_equal(alone[1].view(np.uint32), dist[:12000].view(np.uint32))


@pytest.mark.parametrize("name", sorted(adversarial()))
def test_adversarial_inputs(gpu, name):
    from parsenet_codebase_amd import kernels as K
    P, ks = adversarial(scale=2)[name]
    for k in ks:
        idx, _ = _check(gpu, [P], k, name)
        if P.shape[0] <= 10240:                                       # and the brute-force kernel agrees
            flat = torch.from_numpy(P).to(gpu)
            ragged = K.knn3_ragged(flat, _off([P.shape[0]], gpu), P.shape[0], k, want_dist=True)
            grid = K.knn3_grid(flat, _off([P.shape[0]], gpu), P.shape[0], k, want_dist=True)
            assert torch.equal(grid[0], ragged[0]) and torch.equal(grid[1], ragged[1]), (name, k)
        if name == "copies among random":                             # a copy's neighbours: the 64 first copies
            same = np.flatnonzero((P == np.asarray([0.125, -0.25, 0.375], np.float32)).all(1))
            assert same.size == 3000 and np.array_equal(idx[same], np.tile(same[:64], (same.size, 1)))


def test_short_and_empty_segments_between_others_and_the_batching(gpu):
    rng = np.random.RandomState(8)
    empty = np.zeros((0, 3), np.float32)
    clouds = [rng.uniform(-1, 1, (n, 3)).astype(np.float32) if n else empty for n in (0, 700, 3, 0, 0, 1300, 1, 15, 0)]
    for k in (5, 16):
        idx, dist = _check(gpu, clouds, k, "short and empty")
        for i, r in enumerate(idx[700:703].tolist()):                 # 3 points: all of them, then the point itself
            assert sorted(r[:3]) == [0, 1, 2] and r[3:] == [i] * (k - 3)
        o = 0
        for c in clouds:                                              # alone against in the batch: the same bits
            if c.shape[0]:
                alone = _grid(gpu, [c], k)
                assert np.array_equal(alone[0], idx[o:o + c.shape[0]])
                assert np.array_equal(alone[1].view(np.uint32), dist[o:o + c.shape[0]].view(np.uint32))
            o += c.shape[0]
    assert all(a.shape == (0, 7) for a in _grid(gpu, [empty, empty], 7))


def test_the_argument_contract(gpu):
    from parsenet_codebase_amd import _lib, kernels as K
    lib = load_raw()
    pts = torch.rand(10, 3, device=gpu)
    off = torch.tensor([0, 10], dtype=torch.int32, device=gpu)
    idx = torch.full((10, 8), -77, dtype=torch.int32, device=gpu)
    need = lib.pn_knn3_grid_workspace_bytes(10, 1)
    ws = torch.zeros(need, dtype=torch.uint8, device=gpu)
    real = dict(pts=pts.data_ptr(), off=off.data_ptr(), idx=idx.data_ptr(), ws=ws.data_ptr(), ws_bytes=need,
                stream=_lib.current_stream(gpu))
    check_invalid_arguments(lib, **real)               # (a workspace one byte short among them)
    torch.cuda.synchronize()
    assert bool((idx == -77).all())                    # refused before any launch: the sentinel is untouched
    with pytest.raises(TypeError, match="int32"):
        K.knn3_grid(pts, off.long(), 10, 8)
    with pytest.raises(TypeError, match="float32"):
        K.knn3_grid(pts.double(), off, 10, 8)
    with pytest.raises(ValueError, match=r"\(total,3\)"):
        K.knn3_grid(torch.rand(10, 4, device=gpu), off, 10, 8)
    with pytest.raises(RuntimeError, match="pn_knn3_grid_f32"):
        K.knn3_grid(pts, off, 10, 65)
