"""GPU checks of the ``search`` argument of estimate_normals and orient_normals: "grid" and "auto" give the bits of the
default wherever the default runs — normals, scalars, oriented normals, flips and seeds — for the three layouts; above
the brute-force kernel's 10 240 points "grid" equals point_normals on numpy's brute-force neighbours bit for bit; the
limits that stay, and the argument errors."""
import numpy as np
import pytest
import torch

from tests.test_knn3_grid_gpu import brute
from tests.test_point_normals_abi import angle, sphere

pytestmark = pytest.mark.gpu


def _cloud(n, seed):
    return np.random.RandomState(seed).uniform(-0.5, 0.5, (n, 3)).astype(np.float32)


def _same(a, b):
    """Bit equality of two results: tensors, or tuples / lists of them."""
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and \
            torch.equal(a.view(torch.int32), b.view(torch.int32))
    return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))


def _layouts(gpu):
    single = torch.from_numpy(sphere(700) + 0.01 * _cloud(700, 1)).to(gpu)
    batch = torch.from_numpy(np.stack([_cloud(650, 10 + b) for b in range(3)])).to(gpu)
    ragged = [batch[0], single, torch.from_numpy(_cloud(5, 3)).to(gpu), torch.from_numpy(_cloud(2600, 4)).to(gpu)]
    return single, batch, ragged


@pytest.mark.parametrize("search", ["grid", "auto"])
def test_the_search_does_not_change_a_bit_where_the_default_runs(gpu, search):
    from parsenet_codebase_amd.point_normals import estimate_normals, orient_normals
    for pts in _layouts(gpu):
        for k in (8, 16):
            plain = estimate_normals(pts, k=k, return_scalars=True)
            assert _same(estimate_normals(pts, k=k, return_scalars=True, search=search), plain)
            assert _same(estimate_normals(pts, k=k, search=search), plain[0])
            mst = estimate_normals(pts, k=k, return_scalars=True, orient="mst")
            assert _same(estimate_normals(pts, k=k, return_scalars=True, orient="mst", search=search), mst)
            flags = orient_normals(pts, plain[0], k=k, return_flags=True)
            assert _same(orient_normals(pts, plain[0], k=k, return_flags=True, search=search), flags)
            assert _same(orient_normals(pts, plain[0], k=k, search=search), flags[0])
    view = torch.tensor([0.1, 0.2, 3.0], device=gpu)
    pts = _layouts(gpu)[1]
    assert _same(estimate_normals(pts, viewpoint=view, search=search), estimate_normals(pts, viewpoint=view))


def test_twelve_thousand_points(gpu):
    """A golden-spiral unit sphere of 12 000 points with radial noise 1e-3, k = 16.

    The angle to the analytic radial direction.  tests/test_point_normals_gpu.py asks of its 10 240-point cloud only
    finite normals of non-zero length, so the bar is derived here, from the input alone.  The k neighbours of a point
    lie within its k-th neighbour distance rho (taken from numpy's brute force, not from the code under test): on the
    unit sphere that is a cap of angular radius about rho.  (a) Without noise the points of a cap lie on a circle-
    symmetric bowl of depth rho^2 / 2 whose least-squares plane is perpendicular to the radial direction of the
    neighbours' centroid, which lies inside the cap: at most rho from the query's own direction.  (b) Radial noise of
    standard deviation s tilts the plane fitted to k points of lateral spread rho / 2 per axis by about
    s / (sqrt(k) rho / 2) per axis; six standard deviations on both axes cover 12 000 points.  The bar is
    rho + 6 sqrt(2) * 2 s / (sqrt(k) rho), 0.13 rad for rho = 0.08."""
    from parsenet_codebase_amd import kernels as K
    from parsenet_codebase_amd.point_normals import estimate_normals
    n, k, noise = 12000, 16, 1e-3
    radial = sphere(n).astype(np.float64)
    P = (radial * (1.0 + noise * np.random.RandomState(7).standard_normal((n, 1)))).astype(np.float32)
    pts = torch.from_numpy(P).to(gpu)
    nrm, var, gap = estimate_normals(pts, k=k, return_scalars=True, search="grid")
    idx, d2 = brute(P, k)
    want = K.point_normals(pts, [0, n], torch.from_numpy(idx).to(gpu), k, want_scalars=True)
    assert _same((nrm, var, gap), want)
    assert _same(estimate_normals(pts, k=k, return_scalars=True, search="auto"), want)
    rho = float(np.sqrt(d2[:, -1].astype(np.float64)).max())
    bar = rho + 6.0 * np.sqrt(2.0) * 2.0 * noise / (np.sqrt(k) * rho)
    worst = float(angle(nrm.cpu().numpy(), radial).max())
    print("12 000 points: rho %.4f, bar %.4f rad, worst angle %.4f rad" % (rho, bar, worst))
    assert 0.05 < rho < 0.1 and worst <= bar
    # the list layout above the limit, next to a small cloud
    small = torch.from_numpy(_cloud(300, 5)).to(gpu)
    both = estimate_normals([pts, small], k=k, search="grid")
    assert _same(both[0], nrm) and _same(both[1], estimate_normals(small, k=k))


def test_the_limits_that_stay_and_the_argument_errors(gpu):
    from parsenet_codebase_amd.point_normals import estimate_normals, orient_normals
    big = torch.zeros((10241, 3), device=gpu)
    with pytest.raises(ValueError, match="10240"):
        estimate_normals(big)
    with pytest.raises(ValueError, match="grid"):
        estimate_normals(big)                                         # the message names the way out
    with pytest.raises(ValueError, match="10240"):
        orient_normals(big, big)
    z = torch.zeros((8, 3), device=gpu)
    for bad in ("kd", "brute", "", 0):
        with pytest.raises(ValueError, match="search"):
            estimate_normals(z, search=bad)
        with pytest.raises(ValueError, match="search"):
            orient_normals(z, z, search=bad)
    # orient.hip's own limit is not lifted by the search
    pts = torch.from_numpy(sphere(12000)).to(gpu)
    with pytest.raises(ValueError, match="orients at most"):
        estimate_normals(pts, orient="mst", search="grid")
    with pytest.raises(ValueError, match="orients at most"):
        orient_normals(pts, pts, search="auto")
    assert tuple(estimate_normals(torch.zeros((0, 3), device=gpu), search="grid").shape) == (0, 3)
