"""GPU checks of the global-memory orientation engine (csrc/orient_global.hip): flip, seed and the bits of the normals
against the serial host restatement (tests/native/orient_math_host.cpp) fed the neighbours the GPU itself returned, and
against the one-workgroup kernel wherever that one runs.  The forest is unique, so every comparison is EXACT: there is
no tolerance in this file.  Sizes around the wave, the workgroup (OG_BLOCK) and the stride of a launch (OG_STRIDE),
padded k, ragged batches with empty clouds and boundaries inside a workgroup, the all-ties lattice, a disconnected
cloud, the chain adversary, clouds at and above the one-workgroup limit, engine="auto", determinism and independence of
the layout, estimate_normals end to end on a 20 000-point torus, the argument errors."""
import numpy as np
import pytest
import torch

from tests.test_orient_global_abi import (BLOCK, STRIDE, big_sphere, big_torus, chain, check_chain_precondition,
                                          check_invalid_arguments)
from tests.test_orient_normals_abi import UP, build_harness, host_orient, lattice, same_bits, two_spheres
from tests.test_orient_normals_gpu import _bits, _cloud, _normals

pytestmark = pytest.mark.gpu

LIMIT = 10240
SIZES = (1, 2, 3, 63, 64, 65, 130, 1025, BLOCK - 1, BLOCK, BLOCK + 1)
KS = (1, 3, 5, 16, 64)
EMPTY = np.zeros((0, 3), np.float32)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory.mktemp("omh_global_gpu"))


def _offsets(clouds):
    return np.concatenate([[0], np.cumsum([c.shape[0] for c in clouds])]).astype(np.int32)


def _exact(harness, gpu, clouds, normals, k, what, idx=None):
    """The global engine against the host restatement on the GPU's own neighbours (or on ``idx``), and against the
    one-workgroup kernel when every cloud fits it: every bit.  Returns (normals, flip, seed) as numpy."""
    from parsenet_codebase_amd import kernels as K
    off = _offsets(clouds)
    flat_h = np.concatenate(clouds).astype(np.float32).reshape(-1, 3)
    nin_h = np.concatenate(normals).astype(np.float32).reshape(-1, 3)
    flat, nrm = torch.from_numpy(flat_h).to(gpu), torch.from_numpy(nin_h).to(gpu)
    largest = max(c.shape[0] for c in clouds)
    if idx is None:
        knn3 = K.knn3_ragged if largest <= LIMIT else K.knn3_grid
        idx = knn3(flat, torch.from_numpy(off).to(gpu), max(largest, 1), k)
    else:
        idx = torch.from_numpy(idx).to(gpu)
    out, flip, seed = K.orient_normals_global(flat, off, idx, k, nrm, want_flags=True)
    assert same_bits(_bits(K.orient_normals_global(flat, off, idx, k, nrm)), _bits(out)), what    # without the flags
    n_h, f_h, s_h = host_orient(harness, flat_h, off, idx.cpu().numpy(), nin_h)
    assert np.array_equal(flip.cpu().numpy(), f_h), what
    assert np.array_equal(seed.cpu().numpy(), s_h), what
    assert same_bits(out.cpu().numpy(), n_h), what
    if largest <= LIMIT:
        one = K.orient_normals(flat, off, idx, k, nrm, want_flags=True)
        assert all(same_bits(_bits(a), _bits(b)) for a, b in zip(one, (out, flip, seed))), what
    return out.cpu().numpy(), flip.cpu().numpy(), seed.cpu().numpy()


@pytest.mark.parametrize("k", KS)
def test_engine_against_the_host_restatement_and_the_one_workgroup_kernel(gpu, harness, k):
    """Every size alone (k > N: the padded case; k = 1: no entry), then ragged batches with empty clouds, whose
    boundaries fall inside a workgroup."""
    for n in SIZES:
        _exact(harness, gpu, [_cloud(n, 10 + n)], [_normals(n, n)], k, ("alone", n, k))
    for sizes in ([65], [130, 3], [64, 0, 1, 130, 63], [0, 65, 0]):
        clouds = [_cloud(n, 40 + i) if n else EMPTY for i, n in enumerate(sizes)]
        normals = [_normals(n, 50 + i) if n else EMPTY for i, n in enumerate(sizes)]
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


@pytest.mark.parametrize("n,k", [(STRIDE // 2 - 1, 2), (STRIDE // 2, 2), (STRIDE // 2 + 1, 2),
                                 (STRIDE - 1, 3), (STRIDE, 3), (STRIDE + 1, 3)])
def test_sizes_around_the_stride_of_a_launch(gpu, harness, n, k):
    """n k entries one below, at and one above OG_STRIDE (k = 2), where the lanes of the offer launch begin to stride,
    and n points around OG_STRIDE (k = 3), where those of the per-point launches do."""
    _exact(harness, gpu, [_cloud(n, n % 97)], [_normals(n, n % 89)], k, ("stride", n, k))


def test_the_chain_adversary(gpu, harness):
    """Round one hooks the cloud into one chain of length n - 1: the compress passes really have to walk."""
    P, idx, nrm = chain()
    check_chain_precondition(idx, nrm)
    _exact(harness, gpu, [P], [nrm], 3, "chain", idx=idx)
    _exact(harness, gpu, [P, P[:70], P], [nrm, nrm[:70], -nrm], 3, "chains",
           idx=np.concatenate([idx, chain(70)[1], idx]))


def _signed_sphere(n, seed):
    P, outward = big_sphere(n, seed)
    signs = np.where(np.random.RandomState(seed + 1).uniform(size=n) < 0.5, -1.0, 1.0)[:, None]
    return P, (outward * signs).astype(np.float32), outward


@pytest.mark.parametrize("n", (LIMIT, LIMIT + 1, 12000))
def test_clouds_at_and_above_the_one_workgroup_limit(gpu, harness, n):
    """A jittered sphere at k = 8, the analytic normals under random signs, against the oracle."""
    P, nrm, outward = _signed_sphere(n, 7)
    out, flip, seed = _exact(harness, gpu, [P], [nrm], 8, ("sphere", n))
    print("%d points: %d component(s), %.4f outward" % (n, np.unique(seed).size,
                                                        ((out.astype(np.float64) * outward).sum(1) > 0).mean()))


def test_a_mixed_batch(gpu, harness):
    sizes = [12000, 300, 0, LIMIT + 1]
    parts = [_signed_sphere(n, 20 + i)[:2] if n else (EMPTY, EMPTY) for i, n in enumerate(sizes)]
    _exact(harness, gpu, [p for p, _ in parts], [n for _, n in parts], 8, ("mixed", sizes))


def test_engine_auto_and_layouts(gpu):
    """engine="auto" is engine=None in bits when every cloud fits the one-workgroup kernel, and "global" otherwise; the
    result never depends on the engine, the run or the layout."""
    from parsenet_codebase_amd.point_normals import estimate_normals, orient_normals
    B, N, k = 3, 130, 16
    pts = torch.from_numpy(np.stack([_cloud(N, 30 + b) for b in range(B)])).to(gpu)
    nrm = torch.from_numpy(np.stack([_normals(N, 60 + b) for b in range(B)])).to(gpu)
    none = orient_normals(pts, nrm, k=k, return_flags=True)
    for engine in ("auto", "global"):
        batch = orient_normals(pts, nrm, k=k, return_flags=True, engine=engine)
        again = orient_normals(pts, nrm, k=k, return_flags=True, engine=engine)
        assert tuple(batch[0].shape) == (B, N, 3) and tuple(batch[1].shape) == (B, N) and batch[2].dtype == torch.int32
        assert all(same_bits(_bits(a), _bits(b)) for a, b in zip(batch, again))                # run to run
        assert all(same_bits(_bits(a), _bits(b)) for a, b in zip(batch, none))                 # the engine
        assert same_bits(_bits(orient_normals(pts, nrm, k=k, engine=engine)), _bits(batch[0]))  # without the flags
    ragged, ragged_n = [pts[0], pts[1, :65], pts[2]], [nrm[0], nrm[1, :65], nrm[2]]
    as_list = orient_normals(ragged, ragged_n, k=k, return_flags=True, engine="global")
    assert all(isinstance(o, list) and len(o) == 3 for o in as_list)
    for b in (0, 2):                                                                           # list against batch
        assert all(same_bits(_bits(o[b]), _bits(w[b])) for o, w in zip(as_list, none))
    for b in range(3):                                                                         # alone against batched
        alone = orient_normals(ragged[b], ragged_n[b], k=k, return_flags=True, engine="global")
        assert tuple(alone[0].shape) == (ragged[b].shape[0], 3) and tuple(alone[1].shape) == (ragged[b].shape[0],)
        assert all(same_bits(_bits(a), _bits(o[b])) for a, o in zip(alone, as_list))
    for engine in ("auto", "global"):
        a = estimate_normals(ragged, k=k, orient="mst", engine=engine)
        b = estimate_normals(ragged, k=k, orient="mst")
        assert all(same_bits(_bits(x), _bits(y)) for x, y in zip(a, b))
    # a mixed batch: one cloud above the limit takes the whole call to the global engine
    big, big_n, _ = _signed_sphere(LIMIT + 1, 40)
    mixed = [torch.from_numpy(big).to(gpu), pts[0]]
    mixed_n = [torch.from_numpy(big_n).to(gpu), nrm[0]]
    auto = orient_normals(mixed, mixed_n, k=8, return_flags=True, search="auto", engine="auto")
    glob = orient_normals(mixed, mixed_n, k=8, return_flags=True, search="grid", engine="global")
    assert all(same_bits(_bits(a), _bits(b)) for x, y in zip(auto, glob) for a, b in zip(x, y))
    small = orient_normals(pts[0], nrm[0], k=8, return_flags=True)                             # alone, one workgroup
    assert all(same_bits(_bits(a[1]), _bits(b)) for a, b in zip(auto, small))
    with pytest.raises(ValueError, match="orients at most 10240 points .*engine"):
        orient_normals(mixed, mixed_n, k=8, search="auto")


def test_estimate_normals_end_to_end_on_a_large_torus(gpu, harness):
    """Raw points in, outward normals out, at 20 000 points: estimate_normals(orient="mst", search="auto",
    engine="auto") is orient_normals on its own canonical normals, and the oracle fed the GPU's neighbours."""
    from parsenet_codebase_amd import kernels as K
    from parsenet_codebase_amd.point_normals import estimate_normals, orient_normals
    P, outward = big_torus()
    n, k = P.shape[0], 16
    pts = torch.from_numpy(P).to(gpu)
    canonical = estimate_normals(pts, k=k, search="auto")
    got = estimate_normals(pts, k=k, orient="mst", search="auto", engine="auto")
    again, flip, seed = orient_normals(pts, canonical, k=k, return_flags=True, search="auto", engine="auto")
    assert same_bits(_bits(got), _bits(again))
    assert same_bits(_bits(got), _bits(estimate_normals(pts, k=k, orient="mst", search="grid", engine="global")))
    idx = K.knn3_grid(pts, torch.tensor([0, n], dtype=torch.int32, device=gpu), n, k).cpu().numpy()
    n_h, f_h, s_h = host_orient(harness, P, [0, n], idx, canonical.cpu().numpy())
    assert same_bits(got.cpu().numpy(), n_h) and np.array_equal(flip.cpu().numpy(), f_h)
    assert np.array_equal(seed.cpu().numpy(), s_h)
    before = ((canonical.cpu().numpy().astype(np.float64) * outward).sum(1) > 0).mean()
    after = (got.cpu().numpy().astype(np.float64) * outward).sum(1) > 0
    print("torus, %d points: outward before %.3f, after %.3f" % (n, before, after.mean()))
    assert 0.3 < before < 0.7 and after.all()


def test_the_argument_errors(gpu):
    from parsenet_codebase_amd import _lib
    from parsenet_codebase_amd.point_normals import estimate_normals, orient_normals
    z = torch.zeros((8, 3), device=gpu)
    big = torch.zeros((LIMIT + 1, 3), device=gpu)
    with pytest.raises(ValueError, match="engine must be"):
        orient_normals(z, z, engine="lds")
    with pytest.raises(ValueError, match="without orient"):
        estimate_normals(z, engine="global")
    # search and engine are independent: the brute-force search still refuses the cloud
    with pytest.raises(ValueError, match="brute-force neighbour search takes at most"):
        orient_normals(big, big, engine="global")
    with pytest.raises(ValueError, match="brute-force neighbour search takes at most"):
        estimate_normals(big, orient="mst", engine="global")
    with pytest.raises(ValueError, match="same layout"):
        orient_normals(z, torch.zeros((9, 3), device=gpu), engine="global")
    with pytest.raises(ValueError, match="k must be"):
        orient_normals(z, z, k=65, engine="global")
    empty = torch.zeros((0, 3), device=gpu)
    assert tuple(orient_normals(empty, empty, engine="global").shape) == (0, 3)
    # the C argument checks come before any launch: the output keeps its fill
    lib = _lib.load()
    idx = torch.zeros((8, 8), dtype=torch.int32, device=gpu)
    off = torch.tensor([0, 8], dtype=torch.int32, device=gpu)
    out = torch.full((8, 3), float("nan"), device=gpu)
    ws = torch.zeros(lib.pn_orient_normals_global_workspace_bytes(8, 1), dtype=torch.uint8, device=gpu)
    check_invalid_arguments(lib, pts=z.data_ptr(), off=off.data_ptr(), total=8, max_n=8, idx=idx.data_ptr(),
                            normals_in=z.data_ptr(), normals_out=out.data_ptr(), ws=ws.data_ptr(),
                            stream=_lib.current_stream(gpu))
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and not ws.any()
