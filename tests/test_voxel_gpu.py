"""GPU checks of the voxel-grid downsampling (csrc/voxel.hip, parsenet_codebase_amd/sampling.py): owner, nvox, centroid,
count, first and rep equal to the numpy restatement of the definition (tests.test_voxel_abi.voxel_numpy) on the clouds
and the ragged batch of the CPU tests, on a second run, alone and in a batch, and under a permutation of the points;
voxel_downsample in its three layouts, with gathered per-point arrays, and its errors; the pipeline composed with the
farthest-point sampling.  Every comparison is exact: there is no tolerance in this file."""
import numpy as np
import pytest
import torch

from tests.test_fps_abi import fps_numpy, same
from tests.test_voxel_abi import (LAUNCHES, TILE, cases, cell_map, check_invalid_arguments, check_properties, equal, huge,
                                  load_raw, ragged_batch, raw_call, uniform, voxel_numpy, voxel_numpy_batch)

pytestmark = pytest.mark.gpu


def _off(sizes, gpu):
    return torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)).to(gpu)


def _voxel(gpu, clouds, sizes, origins=None):
    """kernels.voxel_ragged on a ragged batch of numpy clouds -> (owner, nvox, centroid, count, first, rep) as numpy."""
    from parsenet_codebase_amd import kernels as K
    flat = torch.from_numpy(np.concatenate([c.reshape(-1, 3) for c in clouds]).astype(np.float32)).to(gpu)
    vox = torch.from_numpy(np.asarray(sizes, np.float32)).to(gpu)
    org = None if origins is None else torch.from_numpy(np.asarray(origins, np.float32).reshape(-1, 3)).to(gpu)
    out = K.voxel_ragged(flat, _off([c.shape[0] for c in clouds], gpu), vox, org)
    return tuple(o.cpu().numpy() for o in out)


def _check(gpu, clouds, sizes, origins=None, what=""):
    got, want = _voxel(gpu, clouds, sizes, origins), voxel_numpy_batch(clouds, sizes, origins)
    for name, g, w in zip(("owner", "nvox", "centroid", "count", "first", "rep"), got, want):
        assert same(g, w), "%s: %s differs" % (what, name)
    again = _voxel(gpu, clouds, sizes, origins)
    assert all(same(a, b) for a, b in zip(got, again)), "%s: a second run changed a result" % what
    return got


@pytest.mark.parametrize("name", sorted(cases()))
def test_the_kernels_equal_the_definition(gpu, name):
    P, h, origin = cases()[name]
    got = _check(gpu, [P], [h], None if origin is None else [origin], name)
    check_properties(P, h, origin, (got[0], int(got[1][0])) + got[2:])


def test_huge_coordinates(gpu):
    P = huge()
    for h, origin in ((1e38, None), (2.5e38, (0.0, 0.0, 0.0)), (1.0, None), (1e-45, None), (3e38, (-3e38, 3e38, 0.0))):
        _check(gpu, [P], [h], None if origin is None else [origin], "huge, h = %g" % h)


def test_the_ragged_batch_alone_and_in_the_batch(gpu):
    clouds, sizes, origins = ragged_batch()
    for org in (None, origins):
        got = _check(gpu, clouds, sizes, org, "ragged batch")
        assert got[1].tolist()[1:6] == [0, -1, 5, -1, -2] and got[1][0] > 100
        o = 0
        for c, P in enumerate(clouds):
            alone = _voxel(gpu, [P], [sizes[c]], None if org is None else [org[c]])
            n = P.shape[0]
            assert alone[1][0] == got[1][c]
            assert equal([alone[t] for t in (0, 2, 3, 4, 5)], [got[t][o:o + n] for t in (0, 2, 3, 4, 5)])
            o += n
    for bad in (0.0, -1.0, np.inf, np.nan):                       # refused by voxel_downsample; a status down here
        got = _check(gpu, clouds[:4], [0.2, bad, bad, bad], None, "voxel = %r" % bad)
        assert got[1].tolist()[1:] == [-2, -1, -2]
    _check(gpu, [clouds[1], clouds[1]], [0.5, 0.0], None, "empty clouds only")
    _check(gpu, [clouds[1], clouds[3], clouds[1], clouds[1]], [0.5, 0.4, 0.3, 0.2], None, "empty clouds around one")


def test_a_permutation_moves_the_numbering_only(gpu):
    """On the device, where the points of a voxel arrive in any order: 2 049 points over three workgroups."""
    for name in ("uniform 2049, between", "uniform 2049, negative cells", "uniform 2049, one voxel"):
        P, h, origin = cases()[name]
        org = None if origin is None else [origin]
        first = _voxel(gpu, [P], [h], org)
        want = cell_map(P, h, origin, (first[0], int(first[1][0])) + first[2:])
        for seed in (1, 2):
            Q = P[np.random.RandomState(seed).permutation(P.shape[0])]
            got = _voxel(gpu, [Q], [h], org)
            assert cell_map(Q, h, origin, (got[0], int(got[1][0])) + got[2:]) == want, name


def test_wanted_outputs_only(gpu):
    from parsenet_codebase_amd import kernels as K
    P = uniform(1500, 31)
    full = _voxel(gpu, [P], [0.2])
    flat, off, vox = torch.from_numpy(P).to(gpu), _off([1500], gpu), torch.tensor([0.2], device=gpu)
    for want in ((), ("rep",), ("centroid",), ("count", "first"), ("centroid", "rep")):
        out = K.voxel_ragged(flat, off, vox, want=want)
        assert len(out) == 2 + len(want)
        names = ("owner", "nvox") + want
        for name, o in zip(names, out):
            assert same(o.cpu().numpy(), full[("owner", "nvox", "centroid", "count", "first", "rep").index(name)]), name
    with pytest.raises(ValueError, match="want holds"):
        K.voxel_ragged(flat, off, vox, want=("mean",))
    with pytest.raises(ValueError, match="voxel must be"):
        K.voxel_ragged(flat, off, torch.ones(2, device=gpu))
    with pytest.raises(ValueError, match="origin must be"):
        K.voxel_ragged(flat, off, vox, torch.zeros(3, device=gpu))


def test_voxel_downsample_layouts_and_gathers(gpu):
    from parsenet_codebase_amd.sampling import lift, voxel_downsample
    rng = np.random.RandomState(41)
    P = np.stack([uniform(1300, 13), uniform(1300, 14)])
    N = rng.normal(size=P.shape).astype(np.float32)
    L = rng.randint(0, 9, P.shape[:2])
    T, Nt, Lt = (torch.from_numpy(a).to(gpu) for a in (P, N, L))
    h = 0.3
    ref = [voxel_numpy(P[c], h) for c in range(2)]
    cen, own, cnt, rep = voxel_downsample(T, h, return_info=True)                     # a batch: lists
    pnt, nrm, lab, own2 = voxel_downsample(T, h, Nt, Lt, position="point")
    assert all(isinstance(x, list) and len(x) == 2 for x in (cen, cnt, rep, pnt, nrm, lab))
    assert tuple(own.shape) == (2, 1300) and own.dtype == torch.int64 and torch.equal(own, own2)
    for c in range(2):
        o, V, centroid, count, _, r = ref[c]
        assert same(own[c].cpu().numpy(), o.astype(np.int64)) and same(cen[c].cpu().numpy(), centroid[:V])
        assert same(cnt[c].cpu().numpy(), count[:V].astype(np.int64)) and cnt[c].dtype == torch.int64
        assert same(rep[c].cpu().numpy(), r[:V].astype(np.int64)) and rep[c].dtype == torch.int64
        assert torch.equal(pnt[c], T[c][rep[c]]) and torch.equal(nrm[c], Nt[c][rep[c]])
        assert torch.equal(lab[c], Lt[c][rep[c]]) and lab[c].dtype == torch.int64
        assert torch.equal(lift(lab[c], own[c])[rep[c]], lab[c])                       # a representative keeps its label
        # one cloud: tensors
        c1, o1 = voxel_downsample(T[c], h)
        p1, l1, o1b, k1, r1 = voxel_downsample(T[c], h, Lt[c], position="point", return_info=True)
        assert torch.equal(c1, cen[c]) and torch.equal(o1, own[c]) and torch.equal(o1b, own[c])
        assert torch.equal(p1, pnt[c]) and torch.equal(l1, lab[c]) and torch.equal(k1, cnt[c]) and torch.equal(r1, rep[c])
    # a list of clouds of different sizes, a size and an origin per cloud
    sizes, origins = [0.3, 0.2], [(0.1, 0.1, 0.1), (-2.0, 0.0, 0.5)]
    listed = voxel_downsample([T[0], T[1][:900]], sizes, [Nt[0], Nt[1][:900]], origin=origins)
    assert all(isinstance(x, list) and len(x) == 2 for x in listed)
    for c, Pc in enumerate((P[0], P[1][:900])):
        o, V, centroid, _, _, r = voxel_numpy(Pc, sizes[c], origins[c])
        assert same(listed[0][c].cpu().numpy(), centroid[:V]) and same(listed[2][c].cpu().numpy(), o.astype(np.int64))
        assert same(listed[1][c].cpu().numpy(), N[c][r[:V]])
    same_origin = voxel_downsample([T[0], T[1][:900]], np.asarray(sizes), origin=(0.1, 0.1, 0.1))
    assert torch.equal(same_origin[0][0], listed[0][0]) and torch.equal(same_origin[1][0], listed[2][0])


def test_voxel_downsample_errors(gpu):
    from parsenet_codebase_amd.sampling import lift, voxel_downsample
    T = torch.from_numpy(np.stack([uniform(600, 15), uniform(600, 16) * 100])).to(gpu)
    with pytest.raises(ValueError, match="cloud 1: voxel too small"):
        voxel_downsample(T, 1e-5)
    with pytest.raises(ValueError, match="cloud 0: voxel too small"):
        voxel_downsample(T[0], 1e-3, origin=(1e4, 0, 0))
    bad = T[0].clone()
    bad[5, 0] = float("nan")
    red, lab, owner = voxel_downsample(bad, 0.2, torch.arange(600, device=gpu))
    assert tuple(red.shape) == (0, 3) and tuple(lab.shape) == (0,) and (owner == -1).all()
    with pytest.raises(ValueError, match="owner holds -1"):
        lift(lab, owner)
    both = voxel_downsample([bad, T[0]], 0.2)
    assert tuple(both[0][0].shape) == (0, 3) and both[0][1].shape[0] > 10 and (both[1][0] == -1).all()
    with pytest.raises(TypeError, match="float32"):
        voxel_downsample(T.double(), 0.2)
    with pytest.raises(ValueError, match="same layout"):
        voxel_downsample(T, 0.2, torch.zeros(2, 599, device=gpu))
    with pytest.raises(RuntimeError, match="MI355X only"):
        voxel_downsample(T.cpu(), 0.2)


def test_the_pipeline_composed_with_the_farthest_point_sampling(gpu):
    from parsenet_codebase_amd.sampling import lift, reduce_cloud, voxel_downsample
    from tests.test_fps_gpu import _torus
    P = _torus(5000)
    h = 0.08
    own_v, V, _, _, _, rep = voxel_numpy(P, h)
    m = min(500, V)
    assert 500 < V < 5000
    own_f = fps_numpy(P[rep[:V]], m)[2]
    T = torch.from_numpy(P).to(gpu)
    vox, lab_v, o_v = voxel_downsample(T, h, torch.arange(5000, device=gpu), position="point")
    assert same(lab_v.cpu().numpy(), rep[:V].astype(np.int64)) and tuple(vox.shape) == (V, 3)
    red, lab_r, o_f = reduce_cloud(vox, m, lab_v)
    full = lift(lift(torch.arange(m, device=gpu), o_f), o_v)
    assert same(full.cpu().numpy(), own_f[own_v].astype(np.int64))
    assert torch.equal(red, T[lab_r]) and torch.equal(lift(lab_r, o_f)[o_v][lab_r], lab_r)


def test_the_abi_on_the_gpu(gpu):
    from parsenet_codebase_amd import _lib
    lib = load_raw()
    assert lib.pn_voxel_launches() == LAUNCHES
    P = uniform(2 * TILE + 50, 17)
    pts, off, vox = torch.from_numpy(P).to(gpu), _off([P.shape[0]], gpu), torch.tensor([0.25], device=gpu)
    total = P.shape[0]
    need = lib.pn_voxel_workspace_bytes(total, 1)
    ws = torch.zeros(need, dtype=torch.uint8, device=gpu)
    owner = torch.full((total,), -7, dtype=torch.int32, device=gpu)
    nvox = torch.full((1,), -7, dtype=torch.int32, device=gpu)
    real = dict(pts=pts.data_ptr(), off=off.data_ptr(), S=1, total=total, voxel=vox.data_ptr(), owner=owner.data_ptr(),
                nvox=nvox.data_ptr(), ws=ws.data_ptr(), ws_bytes=need)
    check_invalid_arguments(lib, **real)
    torch.cuda.synchronize()
    assert (owner == -7).all() and (nvox == -7).all() and (ws == 0).all()      # refused calls launched nothing
    assert raw_call(lib, **dict(real, stream=_lib.current_stream(gpu))) == 0     # owner and nvox alone
    torch.cuda.synchronize()
    want = voxel_numpy(P, 0.25)
    assert same(owner.cpu().numpy(), want[0]) and nvox.item() == want[1]
