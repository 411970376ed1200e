"""GPU checks of the consistent normal orientation (csrc/orient.hip): flip, seed and the bits of the normals against
the serial host restatement (tests/native/orient_math_host.cpp), which is fed the neighbours the GPU's own knn3_ragged
returned.  The strict order on the edges makes the spanning forest unique, so every comparison is EXACT: there is no
tolerance in this file.  Sizes around the 64-lane wave and the 1 024-thread pass, padded k, ragged batches with empty
clouds, the all-ties lattice, a disconnected cloud, one cloud at the size limit; determinism and independence of the
batch layout; estimate_normals(orient="mst"); the capsule end to end; the argument errors."""
import numpy as np
import pytest
import torch

from tests.test_orient_normals_abi import (UP, build_harness, capsule, check_invalid_arguments, host_orient, lattice,
                                           same_bits, two_spheres)
from tests.test_point_normals_abi import sphere

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 63, 64, 65, 130, 1025)
KS = (3, 5, 16, 64)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory.mktemp("omh_gpu"))


def _cloud(n, seed):
    return np.random.RandomState(seed).uniform(-0.5, 0.5, (n, 3)).astype(np.float32)


def _normals(n, seed):
    """Unit normals from anywhere: random directions, every seventh one the zero normal."""
    v = np.random.RandomState(1000 + seed).standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    v[np.arange(n) % 7 == 3] = 0.0
    return v.astype(np.float32)


def _bits(a):
    return a.detach().cpu().numpy().view(np.uint32)


def _run(gpu, clouds, normals, k):
    """knn3_ragged + orient_normals on a ragged batch of numpy clouds -> (idx, normals, flip, seed) as numpy."""
    from parsenet_codebase_amd import kernels as K
    off = np.concatenate([[0], np.cumsum([c.shape[0] for c in clouds])]).astype(np.int32)
    flat = torch.from_numpy(np.concatenate(clouds).astype(np.float32).reshape(-1, 3)).to(gpu)
    nrm = torch.from_numpy(np.concatenate(normals).astype(np.float32).reshape(-1, 3)).to(gpu)
    idx = K.knn3_ragged(flat, torch.from_numpy(off).to(gpu), max(max(c.shape[0] for c in clouds), 1), k)
    out, flip, seed = K.orient_normals(flat, off, idx, k, nrm, want_flags=True)
    assert same_bits(_bits(K.orient_normals(flat, off, idx, k, nrm)), _bits(out))         # without the flags
    return idx.cpu().numpy(), out.cpu().numpy(), flip.cpu().numpy(), seed.cpu().numpy()


def _exact(harness, gpu, clouds, normals, k, what):
    """The kernel against the host restatement on the kernel's own neighbours: every bit."""
    idx, out, flip, seed = _run(gpu, clouds, normals, k)
    off = np.concatenate([[0], np.cumsum([c.shape[0] for c in clouds])]).astype(np.int32)
    flat = np.concatenate(clouds).astype(np.float32).reshape(-1, 3)
    nin = np.concatenate(normals).astype(np.float32).reshape(-1, 3)
    n_h, f_h, s_h = host_orient(harness, flat, off, idx, nin)
    assert np.array_equal(flip, f_h), what
    assert np.array_equal(seed, s_h), what
    assert same_bits(out, n_h), what
    return out, flip, seed


@pytest.mark.parametrize("k", KS)
def test_kernel_against_the_host_restatement(gpu, harness, k):
    """Every size alone (k > N: the padded case), then ragged batches of 1, 2 and 5 clouds with empty ones."""
    for n in SIZES:
        _exact(harness, gpu, [_cloud(n, 10 + n)], [_normals(n, n)], k, ("alone", n, k))
    empty = np.zeros((0, 3), np.float32)
    for sizes in ([65], [130, 3], [64, 0, 1, 130, 63], [0, 65, 0]):
        clouds = [_cloud(n, 40 + i) if n else empty for i, n in enumerate(sizes)]
        normals = [_normals(n, 50 + i) if n else empty for i, n in enumerate(sizes)]
        _exact(harness, gpu, clouds, normals, k, ("batch", sizes, k))


def test_the_all_ties_lattice_and_a_disconnected_cloud(gpu, harness):
    P = lattice()
    n = P.shape[0]
    down = np.random.RandomState(5).permutation(n) < n // 2
    for k in (5, 16):
        out, flip, seed = _exact(harness, gpu, [P], [np.tile(UP, (n, 1))], k, ("lattice", k))
        assert not flip.any() and not seed.any()
        out, flip, seed = _exact(harness, gpu, [P], [np.where(down[:, None], -UP, UP)], k, ("half negated", k))
        assert np.array_equal(out, np.tile(UP, (n, 1))) and np.array_equal(flip == 1, down) and not seed.any()
    P, outward = two_spheres()
    signs = np.where(np.random.RandomState(6).uniform(size=P.shape[0]) < 0.5, -1.0, 1.0)[:, None]
    out, flip, seed = _exact(harness, gpu, [P], [(outward * signs).astype(np.float32)], 8, "two spheres")
    assert sorted(np.unique(seed).tolist()) == [int(np.argmax(P[:300, 2])), 300 + int(np.argmax(P[300:, 2]))]
    assert ((out.astype(np.float64) * outward).sum(1) > 0).all()
    # duplicated points, and a cloud of zero normals
    base = _cloud(40, 21)
    doubled = np.concatenate([base, base])[np.random.RandomState(0).permutation(80)]
    for k in (3, 16):
        _exact(harness, gpu, [doubled, _cloud(30, 22)], [_normals(80, 23), np.zeros((30, 3), np.float32)], k, "doubled")


def test_one_cloud_at_the_size_limit(gpu, harness):
    """pn_orient_normals_max_points() points of a jittered sphere at k = 8: the analytic normals with random signs."""
    from parsenet_codebase_amd import _lib
    n = _lib.load().pn_orient_normals_max_points()
    outward = sphere(n).astype(np.float64)
    P = (outward * (1.0 + 0.002 * np.random.RandomState(7).standard_normal((n, 1)))).astype(np.float32)
    signs = np.where(np.random.RandomState(8).uniform(size=n) < 0.5, -1.0, 1.0)[:, None]
    out, flip, seed = _exact(harness, gpu, [P], [(outward * signs).astype(np.float32)], 8, "limit")
    print("%d points: %d component(s), %.4f outward" % (n, np.unique(seed).size,
                                                        ((out.astype(np.float64) * outward).sum(1) > 0).mean()))


def test_determinism_and_layout_independence(gpu):
    from parsenet_codebase_amd.point_normals import estimate_normals, orient_normals
    B, N, k = 3, 130, 16
    pts = torch.from_numpy(np.stack([_cloud(N, 30 + b) for b in range(B)])).to(gpu)
    nrm = torch.from_numpy(np.stack([_normals(N, 60 + b) for b in range(B)])).to(gpu)
    batch = orient_normals(pts, nrm, k=k, return_flags=True)
    again = orient_normals(pts, nrm, k=k, return_flags=True)
    assert tuple(batch[0].shape) == (B, N, 3) and tuple(batch[1].shape) == (B, N) and tuple(batch[2].shape) == (B, N)
    assert batch[1].dtype == torch.int32 and batch[2].dtype == torch.int32
    assert all(same_bits(_bits(a), _bits(b)) for a, b in zip(batch, again))                    # run to run
    ragged, ragged_n = [pts[0], pts[1, :65], pts[2]], [nrm[0], nrm[1, :65], nrm[2]]
    as_list = orient_normals(ragged, ragged_n, k=k, return_flags=True)
    assert all(isinstance(o, list) and len(o) == 3 for o in as_list)
    for b in (0, 2):                                                                           # list against batch
        assert all(same_bits(_bits(o[b]), _bits(w[b])) for o, w in zip(as_list, batch))
    for b in range(3):                                                                         # alone against batched
        alone = orient_normals(ragged[b], ragged_n[b], k=k, return_flags=True)
        assert tuple(alone[0].shape) == (ragged[b].shape[0], 3) and tuple(alone[1].shape) == (ragged[b].shape[0],)
        assert all(same_bits(_bits(a), _bits(o[b])) for a, o in zip(alone, as_list))
    assert same_bits(_bits(orient_normals(pts, nrm, k=k)), _bits(batch[0]))                    # without the flags
    # every output row is the input row or its exact negation, as flip says
    want = torch.where(batch[1].bool()[..., None], -nrm, nrm)
    assert same_bits(_bits(want), _bits(batch[0]))
    # estimate_normals: orient=None is the call without the keyword, "mst" is orient_normals on its own result
    plain = estimate_normals(pts, k=k, return_scalars=True)
    none = estimate_normals(pts, k=k, return_scalars=True, orient=None)
    assert all(same_bits(_bits(a), _bits(b)) for a, b in zip(plain, none))
    mst = estimate_normals(pts, k=k, return_scalars=True, orient="mst")
    assert same_bits(_bits(mst[0]), _bits(orient_normals(pts, plain[0], k=k)))
    assert same_bits(_bits(mst[1]), _bits(plain[1])) and same_bits(_bits(mst[2]), _bits(plain[2]))
    assert same_bits(_bits(estimate_normals(pts, k=k, orient="mst")), _bits(mst[0]))
    for layout in (ragged, pts[1]):
        a = estimate_normals(layout, k=k, orient="mst")
        b = orient_normals(layout, estimate_normals(layout, k=k), k=k)
        a, b = (a, b) if isinstance(a, list) else ([a], [b])
        assert all(same_bits(_bits(x), _bits(y)) for x, y in zip(a, b))


def test_the_capsule_end_to_end(gpu):
    """Raw points in, outward normals out: estimate_normals(k=16, orient="mst") on the tilted capsule."""
    from parsenet_codebase_amd.point_normals import estimate_normals
    P, outward = capsule()
    pts = torch.from_numpy(P).to(gpu)
    before = (estimate_normals(pts, k=16).cpu().numpy().astype(np.float64) * outward).sum(1) > 0
    after = (estimate_normals(pts, k=16, orient="mst").cpu().numpy().astype(np.float64) * outward).sum(1) > 0
    print("capsule, %d points: outward before %.3f, after %.3f" % (P.shape[0], before.mean(), after.mean()))
    assert 0.3 < before.mean() < 0.7
    assert after.all()


def test_the_argument_errors(gpu):
    from parsenet_codebase_amd import _lib, kernels
    from parsenet_codebase_amd.point_normals import estimate_normals, orient_normals
    z = torch.zeros((8, 3), device=gpu)
    with pytest.raises(ValueError, match="orient must be"):
        estimate_normals(z, orient="bfs")
    with pytest.raises(ValueError, match="viewpoint"):
        estimate_normals(z, orient="mst", viewpoint=torch.zeros(3, device=gpu))
    with pytest.raises(ValueError, match="10240"):
        orient_normals(torch.zeros((10241, 3), device=gpu), torch.zeros((10241, 3), device=gpu))
    with pytest.raises(ValueError, match="10240"):
        kernels.orient_normals(torch.zeros((10241, 3), device=gpu), [0, 10241],
                               torch.zeros((10241, 3), dtype=torch.int32, device=gpu), 3,
                               torch.zeros((10241, 3), device=gpu))
    with pytest.raises(ValueError, match="same layout"):
        orient_normals(z, torch.zeros((9, 3), device=gpu))
    with pytest.raises(ValueError, match="same layout"):
        orient_normals([z], z)
    with pytest.raises(ValueError, match="float32"):
        orient_normals(z, z.double())
    with pytest.raises(ValueError, match="k must be"):
        orient_normals(z, z, k=0)
    with pytest.raises(ValueError, match="k must be"):
        orient_normals(z, z, k=65)
    with pytest.raises(RuntimeError, match="MI355X only"):
        orient_normals(z, torch.zeros(8, 3))
    assert tuple(orient_normals(torch.zeros((0, 3), device=gpu), torch.zeros((0, 3), device=gpu)).shape) == (0, 3)
    # the C argument checks come before any launch: the output keeps its fill
    lib = _lib.load()
    idx = torch.zeros((8, 8), dtype=torch.int32, device=gpu)
    off = torch.tensor([0, 8], dtype=torch.int32, device=gpu)
    out = torch.full((8, 3), float("nan"), device=gpu)
    check_invalid_arguments(lib, pts=z.data_ptr(), off=off.data_ptr(), total=8, idx=idx.data_ptr(),
                            normals_in=z.data_ptr(), normals_out=out.data_ptr(), stream=_lib.current_stream(gpu))
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
