"""GPU checks of the seams between the raw-cloud kernels (parsenet_codebase_amd/ragged.py, csrc/ragged.h): one ragged
batch with empty clouds at both ends and in a run and sizes on both sides of the FPS tile through ``knn3_grid``,
``orient_normals_global`` and ``fps_ragged``, the offsets given in the form each wrapper has always taken and as a
``Clouds`` — every output equal to the other form and to that cloud run alone —, and the number of host-to-device
copies of ``estimate_normals(orient="mst")`` and ``reduce_cloud``.  Every comparison is exact."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [0, 0, 1, 1023, 0, 1024, 1025, 0]      # FPS_TILE = 1024 points
K8 = 8


def _clouds(gpu, sizes, seed=3):
    rng = np.random.RandomState(seed)
    return [torch.from_numpy(rng.uniform(-1, 1, (n, 3)).astype(np.float32)).to(gpu) for n in sizes]


def _same(a, b):
    """Equality of every bit of two int32 or fp32 tensors (a NaN, the radius of a sample never chosen, equals itself)."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32),
                                                                     b.contiguous().view(torch.int32))


def test_both_forms_of_the_offsets_and_every_cloud_alone(gpu):
    from parsenet_codebase_amd import kernels as K
    from parsenet_codebase_amd.point_normals import estimate_normals
    from parsenet_codebase_amd.ragged import Clouds
    parts = _clouds(gpu, SIZES)
    c = Clouds(parts, "test")
    host = np.concatenate([[0], np.cumsum(SIZES)])
    dev = torch.from_numpy(host.astype(np.int32)).to(gpu)
    assert c.off.tolist() == host.tolist() and torch.equal(c.device_offsets(), dev)
    assert c.device_offsets() is c.device_offsets()
    normals = torch.cat(estimate_normals(parts, k=K8, search="grid"))
    for other in (c.flat[:-1], torch.zeros((c.total + 1, 3), device=gpu)):      # not the array the Clouds flattened
        with pytest.raises(ValueError, match="not the flat array"):
            K.knn3_grid(other, c, None, K8)
        with pytest.raises(ValueError, match="ascend from 0"):
            K.orient_normals_global(other, c, torch.zeros((other.shape[0], K8), dtype=torch.int32, device=gpu), K8, other)

    idx, dist = K.knn3_grid(c.flat, dev, max(SIZES), K8, want_dist=True)
    assert all(_same(a, b) for a, b in zip((idx, dist), K.knn3_grid(c.flat, c, None, K8, want_dist=True)))
    oriented = K.orient_normals_global(c.flat, host, idx, K8, normals, want_flags=True)
    assert all(_same(a, b) for a, b in zip(oriented, K.orient_normals_global(c.flat, c, idx, K8, normals,
                                                                            want_flags=True)))
    start = torch.tensor([0, 3, 0, 1000, 2, 1023, 1024, 0], dtype=torch.int32, device=gpu)
    fps = K.fps_ragged(c.flat, dev, max(SIZES), 5, start=start, want_owner=True, want_radius=True)
    assert all(_same(a, b) for a, b in zip(fps, K.fps_ragged(c.flat, c, None, 5, start=start, want_owner=True,
                                                             want_radius=True)))
    sample, owner, fdist, radius = fps
    assert (sample[[0, 1, 4, 7]] == -1).all() and (sample[2] == torch.tensor([0, -1, -1, -1, -1], device=gpu)).all()
    assert (sample[[3, 5, 6]] >= 0).all() and sample[:, 0].tolist() == [-1, -1, 0, 1000, -1, 1023, 1024, -1]

    for s, (P, n) in enumerate(zip(parts, SIZES)):
        rows = slice(int(host[s]), int(host[s + 1]))
        one = torch.tensor([0, n], dtype=torch.int32, device=gpu)
        a_sample, a_owner, a_fdist, a_radius = K.fps_ragged(P, one, n, 5, start=start[s:s + 1], want_owner=True,
                                                            want_radius=True)
        assert _same(a_sample[0], sample[s]) and _same(a_radius[0], radius[s]), s
        assert _same(a_owner, owner[rows]) and _same(a_fdist, fdist[rows]), s
        if n == 0:
            continue
        a_idx, a_dist = K.knn3_grid(P, one, n, K8, want_dist=True)
        assert _same(a_idx, idx[rows]) and _same(a_dist, dist[rows]), s
        alone = K.orient_normals_global(P, [0, n], a_idx, K8, normals[rows], want_flags=True)
        assert all(_same(a, b[rows]) for a, b in zip(alone, oriented)), s


@pytest.fixture
def uploads(monkeypatch):
    """The host-to-device copies made through ``_lib.h2d`` while the test runs: a list of their shapes."""
    from parsenet_codebase_amd import _lib
    seen, h2d = [], _lib.h2d

    def counted(array, device):
        seen.append(np.shape(array))
        return h2d(array, device)
    monkeypatch.setattr(_lib, "h2d", counted)
    return seen


def test_estimate_normals_uploads_the_offsets_once(gpu, uploads):
    from parsenet_codebase_amd import kernels as K
    from parsenet_codebase_amd.point_normals import estimate_normals
    sizes = [1, 70, 300]
    parts = _clouds(gpu, sizes, seed=4)
    got = estimate_normals(parts, orient="mst", search="grid", engine="global")
    assert len(uploads) <= 2, uploads                              # the offsets and the tile table
    flat, host = torch.cat(parts), np.concatenate([[0], np.cumsum(sizes)])
    idx = K.knn3_grid(flat, torch.from_numpy(host.astype(np.int32)).to(gpu), max(sizes), 16)
    want = K.orient_normals_global(flat, host, idx, 16, K.point_normals(flat, host, idx, 16))
    assert [tuple(g.shape) for g in got] == [(n, 3) for n in sizes] and torch.equal(torch.cat(got), want)
    # the forms that copied less before copy no more now: host integers ride with the tile table, nothing to do or a
    # refused cloud copies nothing
    del uploads[:]
    K.point_normals(flat, host, idx, 16)
    assert len(uploads) == 1, uploads
    del uploads[:]
    empty = torch.zeros((0, 3), device=gpu)
    assert tuple(estimate_normals(empty, orient="mst", search="grid", engine="global").shape) == (0, 3)
    assert tuple(estimate_normals(torch.zeros((0, 5, 3), device=gpu), orient="mst").shape) == (0, 5, 3)
    assert tuple(K.point_normals(empty, [0], torch.zeros((0, 16), dtype=torch.int32, device=gpu), 16).shape) == (0, 3)
    big = torch.zeros((10241, 3), device=gpu)
    with pytest.raises(ValueError, match="orients at most"):
        K.orient_normals(big, [0, 10241], torch.zeros((10241, 3), dtype=torch.int32, device=gpu), 3, big)
    assert uploads == []


def test_reduce_cloud_uploads_the_offsets_once(gpu, uploads):
    from parsenet_codebase_amd import kernels as K
    from parsenet_codebase_amd.sampling import reduce_cloud
    sizes = [1, 70, 300]
    parts = _clouds(gpu, sizes, seed=5)
    labels = [torch.arange(n, device=gpu) * 10 for n in sizes]
    start = [0, 69, 150]
    reduced, labels_r, owner = reduce_cloud(parts, 1, labels, start=start)
    assert len(uploads) <= 2, uploads                              # the offsets and the starts
    flat, host = torch.cat(parts), np.concatenate([[0], np.cumsum(sizes)])
    sample, k_owner, _ = K.fps_ragged(flat, torch.from_numpy(host.astype(np.int32)).to(gpu), max(sizes), 1,
                                      start=torch.tensor(start, dtype=torch.int32, device=gpu), want_owner=True)
    assert sample[:, 0].tolist() == start
    from parsenet_codebase_amd.sampling import farthest_point_sample
    for call in (farthest_point_sample, reduce_cloud):              # a batch of no clouds: refused, as it always was
        with pytest.raises(ValueError):
            call(torch.zeros((0, 5, 3), device=gpu), 2)
    for s in range(3):
        assert torch.equal(reduced[s], parts[s][start[s]:start[s] + 1])
        assert labels_r[s].tolist() == [10 * start[s]]
        assert torch.equal(owner[s], k_owner[int(host[s]):int(host[s + 1])].long())
