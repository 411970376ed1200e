"""GPU checks of the k-NN PCA point normals: csrc/normals.hip against the host compile of the same header at the
smallest shapes at which tiling can go wrong, robustness and the argument contract, determinism and independence of
the batch layout, one end-to-end use (the cylinder fit) and the size limit."""
import numpy as np
import pytest
import torch

from tests.test_point_normals_abi import (BAR, GAP_ABS, GAP_MIN, SCALAR_REL, VARIATION_ABS, angle, build_harness,
                                          check_invalid_arguments, cylinder, header, load_raw, reference)

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 63, 64, 65, 130)
KS = (3, 5, 16, 64)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory.mktemp("nmh_gpu"))


def _cloud(n, seed):
    return np.random.RandomState(seed).uniform(-0.5, 0.5, (n, 3)).astype(np.float32)


def _bits(a):
    return a.detach().cpu().numpy().view(np.uint32)


def _run(gpu, clouds, k, view=None):
    """knn3_ragged + point_normals on a ragged batch of numpy clouds -> (idx, normals, variation, gap) as numpy."""
    from parsenet_codebase_amd import kernels as K
    off = np.concatenate([[0], np.cumsum([c.shape[0] for c in clouds])]).astype(np.int32)
    flat = torch.from_numpy(np.concatenate(clouds).astype(np.float32).reshape(-1, 3)).to(gpu)
    idx = K.knn3_ragged(flat, torch.from_numpy(off).to(gpu), max(max(c.shape[0] for c in clouds), 1), k)
    view_d = None if view is None else torch.from_numpy(np.asarray(view, np.float32)).to(gpu)
    nrm, var, gap = K.point_normals(flat, off, idx, k, viewpoints=view_d, want_scalars=True)
    return idx.cpu().numpy(), nrm.cpu().numpy(), var.cpu().numpy(), gap.cpu().numpy()


def _against_header(harness, gpu, clouds, k, what, view=None):
    """The kernel against the host compile on the kernel's own neighbours.  Returns (bit-identical values, values)."""
    idx, nrm, var, gap = _run(gpu, clouds, k, view)
    off = np.concatenate([[0], np.cumsum([c.shape[0] for c in clouds])]).astype(np.int32)
    flat = np.concatenate(clouds).astype(np.float32).reshape(-1, 3)
    n_h, v_h, g_h = header(harness, flat, off, idx, view=view)
    assert np.isfinite(nrm).all() and np.isfinite(var).all() and np.isfinite(gap).all(), what
    zero = ~n_h.any(1)
    small = np.repeat(np.diff(off) < 3, np.diff(off))
    assert zero[small].all(), what
    assert np.array_equal(~nrm.any(1), zero), what                      # (0,0,0) exactly where the definition says
    assert not var[zero].any() and not gap[zero].any(), what
    assert (np.abs(var.astype(np.float64) - v_h) <= VARIATION_ABS + SCALAR_REL * np.abs(v_h)).all(), what
    assert (np.abs(gap.astype(np.float64) - g_h) <= GAP_ABS + SCALAR_REL * np.abs(g_h)).all(), what
    enters = ~zero & (g_h >= GAP_MIN)
    worst = float(angle(nrm[enters], n_h[enters]).max(initial=0.0))
    assert worst <= BAR, (what, worst)
    if view is None:      # same sign too, not only the same line
        assert ((nrm[enters].astype(np.float64) * n_h[enters]).sum(1) > 0).all(), what
    got = np.concatenate([nrm.reshape(-1), var, gap]).view(np.uint32)
    want = np.concatenate([n_h.reshape(-1), v_h, g_h]).view(np.uint32)
    return int((got == want).sum()), got.shape[0]


@pytest.mark.parametrize("k", KS)
def test_kernel_against_the_host_compiled_header(gpu, harness, k):
    """Every size alone (k > N: the padded case), then ragged batches of 1, 2 and 5 unequal segments with an empty
    one among them.  Bit-identical outputs are counted and printed (all of them are expected to be), the bar is
    what is asserted."""
    same = count = 0
    for n in SIZES:
        s, c = _against_header(harness, gpu, [_cloud(n, 10 + n)], k, ("alone", n, k))
        same, count = same + s, count + c
    empty = np.zeros((0, 3), np.float32)
    for clouds in ([_cloud(65, 1)], [_cloud(130, 2), _cloud(3, 3)],
                   [_cloud(64, 4), empty, _cloud(1, 5), _cloud(130, 6), _cloud(63, 7)], [empty, _cloud(65, 8), empty]):
        view = np.random.RandomState(len(clouds)).uniform(-2, 2, (len(clouds), 3)).astype(np.float32)
        for v in (None, view):
            s, c = _against_header(harness, gpu, clouds, k, ("batch", len(clouds), k, v is not None), view=v)
            same, count = same + s, count + c
    print("k = %d: %d of %d output values bit-identical to the host compile" % (k, same, count))


def test_kernel_against_numpy_eigh(gpu):
    """The kernel against the float64 restatement itself, on the noisy cylinder (400 points, 7 tiles)."""
    P, _ = cylinder(400, seed=9, noise=1e-3)
    for k in (5, 16):
        idx, nrm, var, gap = _run(gpu, [P], k)
        n_r, v_r, g_r, _ = reference(P, idx)
        enters = g_r >= GAP_MIN
        assert enters.mean() >= 0.98
        assert angle(nrm[enters], n_r[enters]).max() <= BAR
        assert (np.abs(var - v_r) <= VARIATION_ABS + SCALAR_REL * np.abs(v_r)).all()
        assert (np.abs(gap - g_r) <= GAP_ABS + SCALAR_REL * np.abs(g_r)).all()


def test_duplicates_coincident_points_and_the_argument_contract(gpu, harness):
    from parsenet_codebase_amd import _lib
    base = _cloud(40, 21)
    doubled = np.concatenate([base, base])[np.random.RandomState(0).permutation(80)]
    point = np.tile(np.asarray([[0.25, -0.5, 0.125]], np.float32), (70, 1))
    for k in (3, 16, 64):
        _against_header(harness, gpu, [doubled, point, _cloud(2, 22)], k, ("duplicates", k))
        _, nrm, var, gap = _run(gpu, [doubled, point, _cloud(2, 22)], k)
        assert not nrm[80:].any() and not var[80:].any() and not gap[80:].any()     # coincident, and two points
        assert nrm[:80].any(1).all()                          # (k = 3 of a doubled cloud: a line, still a direction)
    # the argument checks come before any launch: the output keeps its fill
    lib = load_raw()
    pts = torch.from_numpy(_cloud(10, 1)).to(gpu)
    idx = torch.zeros((10, 8), dtype=torch.int32, device=gpu)
    table = torch.tensor([0, 10, 0, 0], dtype=torch.int32, device=gpu)
    out = torch.full((10, 3), float("nan"), device=gpu)
    real = dict(pts=pts.data_ptr(), off=table.data_ptr(), idx=idx.data_ptr(), tile_seg=table[2:].data_ptr(),
                tile_first=table[3:].data_ptr(), normals=out.data_ptr(), stream=_lib.current_stream(gpu))
    check_invalid_arguments(lib, **real)
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


def test_determinism_and_layout_independence(gpu):
    from parsenet_codebase_amd.point_normals import estimate_normals
    B, N, k = 3, 130, 16
    pts = torch.from_numpy(np.stack([_cloud(N, 30 + b) for b in range(B)])).to(gpu)
    batch = estimate_normals(pts, k=k, return_scalars=True)
    again = estimate_normals(pts, k=k, return_scalars=True)
    assert tuple(batch[0].shape) == (B, N, 3) and tuple(batch[1].shape) == (B, N) and tuple(batch[2].shape) == (B, N)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(batch, again))               # run to run
    ragged = [pts[0], pts[1, :65], pts[2]]
    as_list = estimate_normals(ragged, k=k, return_scalars=True)
    assert all(isinstance(o, list) and len(o) == 3 for o in as_list)
    for b in (0, 2):                                                                           # list against batch
        assert all(np.array_equal(_bits(o[b]), _bits(w[b])) for o, w in zip(as_list, batch))
    for b, cloud in enumerate(ragged):                                                         # alone against batched
        alone = estimate_normals(cloud, k=k, return_scalars=True)
        assert tuple(alone[0].shape) == (cloud.shape[0], 3) and tuple(alone[1].shape) == (cloud.shape[0],)
        assert all(np.array_equal(_bits(a), _bits(o[b])) for a, o in zip(alone, as_list))
    assert np.array_equal(_bits(estimate_normals(pts, k=k)), _bits(batch[0]))                  # without the scalars
    # canonical sign against a viewpoint: the same normals, flipped exactly where n . (v - p) < 0 in float64
    view = torch.tensor([[0.1, 0.2, 3.0], [-2.0, 0.5, 0.1], [0.0, 0.0, 0.0]], device=gpu)
    plain = batch[0].cpu().numpy()
    lead = np.take_along_axis(plain, np.argmax(np.abs(plain), 2)[..., None], 2)
    assert (lead > 0).all()
    d = view.cpu().numpy().astype(np.float64)[:, None, :] - pts.cpu().numpy().astype(np.float64)
    n64 = plain.astype(np.float64)
    dot = (n64[..., 0] * d[..., 0] + n64[..., 1] * d[..., 1]) + n64[..., 2] * d[..., 2]
    want = np.where((dot < 0)[..., None], -plain, plain)
    assert 0.2 < (dot < 0).mean() < 0.8
    for v in (view, [view[0], view[1], view[2]]):
        seen = estimate_normals(pts, k=k, viewpoint=v, return_scalars=True)
        assert np.array_equal(seen[0].cpu().numpy(), want)
        assert np.array_equal(_bits(seen[1]), _bits(batch[1])) and np.array_equal(_bits(seen[2]), _bits(batch[2]))
    one = estimate_normals(pts, k=k, viewpoint=view[0])                                        # (3,): every cloud
    assert np.array_equal(one[0].cpu().numpy(), want[0])
    assert np.array_equal(estimate_normals(pts[1], k=k, viewpoint=view[1]).cpu().numpy(), want[1])


def _axis64(normals):
    """The fp64 restatement of the cylinder fit's axis (src/primitive_forward.py:784-790 with unit weights): the
    right singular vector of the smallest singular value of the normals."""
    return np.linalg.svd(np.asarray(normals, np.float64), full_matrices=False)[2][-1]


def test_estimated_normals_feed_the_cylinder_fit(gpu):
    """400 points of a cylinder with noise 1e-3: the batched cylinder fit on the ESTIMATED, unoriented normals returns
    the axis it returns on the analytic normals, to within twice the angle the fp64 restatement shows between its
    own two axes (the factor 2 is for the fp32 fit).  The test is well-posed because that fit is sign-invariant: the
    axis is the smallest singular vector of the normals, and flipping rows of a matrix does not change its right
    singular vectors — canonical-sign normals are as good as outward ones here.
    Measured: restatement 2.683e-3 rad (bound 5.366e-3), fit on the GPU 2.683e-3 rad."""
    from parsenet_codebase_amd.fitting import Fit
    from parsenet_codebase_amd.point_normals import estimate_normals
    P, analytic = cylinder(400, seed=9, noise=1e-3)
    idx = _run(gpu, [P], 16)[0]
    a0, a1 = _axis64(analytic), _axis64(reference(P, idx)[0])
    bound = 2.0 * float(angle(a0[None], a1[None])[0])
    pts = torch.from_numpy(P).to(gpu)
    est = estimate_normals(pts, k=16)
    assert ((est.cpu().numpy() * analytic).sum(1) < 0).mean() > 0.2          # unoriented indeed: many point inwards
    w = torch.ones((P.shape[0], 1), device=gpu)
    g0 = Fit().fit_cylinder_torch(pts, torch.from_numpy(analytic).to(gpu), w)[0].cpu().numpy().reshape(1, 3)
    g1 = Fit().fit_cylinder_torch(pts, est, w)[0].cpu().numpy().reshape(1, 3)
    got = float(angle(g0, g1)[0])
    print("axis angle: restatement %.3e rad, bound %.3e, fit on the GPU %.3e" % (bound / 2, bound, got))
    assert angle(g0, np.asarray([[1.0, 2.0, 2.0]]) / 3.0)[0] < 1e-2          # and it is the cylinder's axis
    assert 0 < bound < 0.02
    assert got <= bound


def test_the_size_limit_and_the_argument_errors(gpu):
    from parsenet_codebase_amd.point_normals import estimate_normals
    with pytest.raises(ValueError, match="10240"):
        estimate_normals(torch.zeros((10241, 3), device=gpu))
    with pytest.raises(ValueError, match="10240"):
        estimate_normals([torch.zeros((8, 3), device=gpu), torch.zeros((10241, 3), device=gpu)])
    with pytest.raises(ValueError, match="float32"):
        estimate_normals(torch.zeros((8, 3), device=gpu, dtype=torch.float64))
    with pytest.raises(ValueError, match="k must be"):
        estimate_normals(torch.zeros((8, 3), device=gpu), k=2)
    with pytest.raises(ValueError, match="k must be"):
        estimate_normals(torch.zeros((8, 3), device=gpu), k=65)
    with pytest.raises(ValueError, match=r"\(N,3\)"):
        estimate_normals(torch.zeros((8, 4), device=gpu))
    with pytest.raises(ValueError, match="viewpoint"):
        estimate_normals(torch.zeros((2, 8, 3), device=gpu), viewpoint=torch.zeros((3, 3), device=gpu))
    with pytest.raises(RuntimeError, match="MI355X only"):
        estimate_normals(torch.zeros((8, 3), device=gpu), viewpoint=torch.zeros(3))
    # the largest cloud the search takes goes through, and an empty one gives an empty result
    big = estimate_normals(torch.from_numpy(_cloud(10240, 3)).to(gpu), k=8)
    assert tuple(big.shape) == (10240, 3) and bool(torch.isfinite(big).all()) and bool(big.abs().sum(1).gt(0.5).all())
    assert tuple(estimate_normals(torch.zeros((0, 3), device=gpu)).shape) == (0, 3)
