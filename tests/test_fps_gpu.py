"""GPU checks of the farthest-point sampling (csrc/fps.hip, parsenet_codebase_amd/sampling.py): sample, radius, owner and
dist equal to the numpy restatement of the definition (tests.test_fps_abi.fps_numpy) at every size around the wave and
the tile, on ragged batches, on ties that span workgroups, on the adversarial clouds, with every kind of start and with
non-finite input; one larger cloud by the three exact properties and a torch brute force; the purpose (a smaller
covering radius than a prefix or a random choice); reduce_cloud and lift; the argument contract.  Every comparison
is exact: there is no tolerance in this file."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests.test_fps_abi import (ROOT, TILE, check_invalid_arguments, check_properties, fps_numpy, fps_numpy_batch,
                                load_raw, same, tied_candidates)
from tests.test_knn3_grid_abi import collinear, copies_among_random, lattice, offset_cloud, planar

pytestmark = pytest.mark.gpu


def _off(sizes, gpu):
    return torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)).to(gpu)


def _fps(gpu, clouds, m, start=None):
    """kernels.fps_ragged on a ragged batch of numpy clouds -> (sample, radius, owner, dist) as numpy."""
    from parsenet_codebase_amd import kernels as K
    sizes = [c.shape[0] for c in clouds]
    flat = torch.from_numpy(np.concatenate([c.reshape(-1, 3) for c in clouds]).astype(np.float32)).to(gpu)
    st = None if start is None else torch.tensor(start, dtype=torch.int32, device=gpu)
    sample, owner, dist, radius = K.fps_ragged(flat, _off(sizes, gpu), max(max(sizes), 1), m, start=st, want_owner=True,
                                               want_radius=True)
    return sample.cpu().numpy(), radius.cpu().numpy(), owner.cpu().numpy(), dist.cpu().numpy()


def _check(gpu, clouds, m, start=None, what=""):
    got, want = _fps(gpu, clouds, m, start), fps_numpy_batch(clouds, m, start)
    for name, g, w in zip(("sample", "radius", "owner", "dist"), got, want):
        assert same(g, w), "%s: %s differs (m = %d)" % (what, name, m)
    return got


def _uniform(n, seed):
    return np.random.RandomState(seed).uniform(-1, 1, (n, 3)).astype(np.float32)


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 5000])
def test_every_size_around_the_wave_and_the_tile(gpu, n):
    P = _uniform(n, n)
    for m in sorted({m for m in (1, 2, 17, n - 1, n, n + 5) if m >= 1}):
        _check(gpu, [P], m, what="n = %d" % n)


def test_ragged_batches_alone_in_a_batch_and_on_a_second_run(gpu):
    five = [_uniform(TILE + 300, 1), np.zeros((0, 3), np.float32), _uniform(7, 2), _uniform(2 * TILE, 3),
            _uniform(40, 4)]
    m = 23                                                       # the 7-point cloud is shorter than m, one is empty
    for batch in ([five[0]], [five[2], five[3]], five, [five[1]], [five[1], five[4], five[1]]):
        got = _check(gpu, batch, m, what="batch of %d" % len(batch))
        again = _fps(gpu, batch, m)
        assert all(same(a, b) for a, b in zip(got, again)), "a second run changed a result"
        o = 0
        for c, P in enumerate(batch):
            alone = _fps(gpu, [P], m)
            n = P.shape[0]
            assert same(alone[0][0], got[0][c]) and same(alone[1][0], got[1][c])
            assert same(alone[2], got[2][o:o + n]) and same(alone[3], got[3][o:o + n])
            o += n
    assert (got[0][0] == -1).all() and (got[0][2] == -1).all() and np.isnan(got[1][0]).all()


def test_the_three_layouts_agree(gpu):
    from parsenet_codebase_amd.sampling import farthest_point_sample
    P = np.stack([_uniform(1500, 5), _uniform(1500, 6)])
    T = torch.from_numpy(P).to(gpu)
    m = 33
    batch = farthest_point_sample(T, m, return_owner=True, return_radius=True)
    assert [tuple(b.shape) for b in batch] == [(2, m), (2, 1500), (2, 1500), (2, m)]
    assert [b.dtype for b in batch] == [torch.int64, torch.int64, torch.float32, torch.float32]
    listed = farthest_point_sample([T[0], T[1]], m, return_owner=True, return_radius=True)
    for c in range(2):
        single = farthest_point_sample(T[c], m, return_owner=True, return_radius=True)
        want = fps_numpy(P[c], m)
        for b, l, s, w in zip(batch, listed, single, (want[0], want[2], want[3], want[1])):
            assert torch.equal(b[c], s) and torch.equal(l[c], s)
            assert same(s.cpu().numpy().astype(w.dtype), w)
    sample = farthest_point_sample(T[0], m)
    assert torch.equal(sample, batch[0][0]) and tuple(T[0][sample].shape) == (m, 3)


def test_ties_on_the_lattice_go_to_the_lowest_index_across_workgroups(gpu):
    P = lattice(16)                                              # 4 096 points, four workgroups, every step a tie
    got = _check(gpu, [P], 64, what="lattice")
    spans = 0
    for t in range(1, 9):
        tied = tied_candidates(P, got[0][0][:t])
        assert got[0][0][t] == tied[0]
        spans += len(tied) > 1 and tied[-1] // TILE > tied[0] // TILE
    assert spans >= 4                                            # ties between points of different workgroups


@pytest.mark.parametrize("name", ["copies among random", "offset, 1e-4 spacing", "planar", "collinear"])
def test_adversarial_clouds(gpu, name):
    P = {"copies among random": lambda: copies_among_random(600, 400), "offset, 1e-4 spacing": lambda: offset_cloud(1500),
         "planar": lambda: planar(1300), "collinear": lambda: collinear(1100)}[name]()
    for m in (50, 450):                                          # 450: the 600 copies are chosen after everything else
        got = _check(gpu, [P], m, what=name)
    if name == "copies among random":
        copies = np.flatnonzero((P == np.asarray([0.125, -0.25, 0.375], np.float32)).all(1))
        assert len(copies) == 600 and np.isin(got[0][0][:401], copies).sum() == 1
        assert np.isin(got[0][0][401:], copies).all() and (got[1][0][401:] == 0).all()


def test_start_as_an_int_per_cloud_and_out_of_range(gpu):
    from parsenet_codebase_amd.sampling import farthest_point_sample
    clouds = [_uniform(300, 7), _uniform(TILE + 5, 8), _uniform(9, 9)]
    for start in ([5, 1000, 3], [-7, 10 ** 6, 9], [299, TILE + 4, 0]):
        _check(gpu, clouds, 12, start, what="start %r" % (start,))
    T = [torch.from_numpy(c).to(gpu) for c in clouds]
    for start, each in ((None, [0, 0, 0]), (4, [4, 4, 4]), ([5, 1000, 3], [5, 1000, 3]), (10 ** 12, [299, TILE + 4, 8]),
                        (np.asarray([1, 2, -3]), [1, 2, 0])):
        got = farthest_point_sample(T, 12, start=start)
        for g, P, s in zip(got, clouds, each):
            assert same(g.cpu().numpy().astype(np.int32), fps_numpy(P, 12, s)[0])
    assert same(farthest_point_sample(T[0], 5, start=77).cpu().numpy().astype(np.int32), fps_numpy(clouds[0], 5, 77)[0])


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
def test_a_non_finite_cloud_inside_a_batch(gpu, value):
    bad = _uniform(TILE + 50, 10)
    bad[TILE + 20, 1] = value
    clouds = [_uniform(500, 11), bad, _uniform(1200, 12)]
    got = _check(gpu, clouds, 20, what="non-finite")
    assert (got[0][1] == -1).all() and np.isnan(got[1][1]).all()
    assert (got[2][500:500 + TILE + 50] == -1).all() and np.isnan(got[3][500:500 + TILE + 50]).all()
    clean = _fps(gpu, [clouds[0], clouds[2]], 20)
    assert same(clean[0], got[0][[0, 2]]) and same(clean[2], np.concatenate([got[2][:500], got[2][-1200:]]))


def _torus(n):
    spec = importlib.util.spec_from_file_location("orient_normals_ab", os.path.join(ROOT, "tools", "orient_normals_ab.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.jittered_torus(n)[0]


def _nearest_sample(T, Q, rows=16384):
    """(first-minimum argmin, minimum) over the samples Q of ((dx*dx + dy*dy) + dz*dz) in fp32, chunked over T.  The
    first minimum is taken as the smallest rank that attains the minimum: an integer minimum, whatever torch's argmin
    does on ties."""
    rank = torch.arange(Q.shape[0], device=T.device)
    arg, val = [], []
    for a in range(0, T.shape[0], rows):
        dx, dy, dz = (T[a:a + rows, None, c] - Q[None, :, c] for c in range(3))
        d = (dx * dx + dy * dy) + dz * dz
        v = d.min(1).values
        arg.append(torch.where(d == v[:, None], rank[None, :], Q.shape[0]).min(1).values)
        val.append(v)
    return torch.cat(arg), torch.cat(val)


def test_a_hundred_thousand_points_by_the_three_properties_and_brute_force(gpu):
    from parsenet_codebase_amd.sampling import farthest_point_sample
    P = _torus(100000)
    T = torch.from_numpy(P).to(gpu)
    m = 512
    sample, owner, dist, radius = farthest_point_sample(T, m, return_owner=True, return_radius=True)
    s, o, d, r = (x.cpu().numpy() for x in (sample, owner, dist, radius))
    check_properties(P, s.astype(np.int32), r, d)
    arg, val = _nearest_sample(T, T[sample])
    assert torch.equal(arg, owner) and torch.equal(val, dist)
    assert same(s[:40].astype(np.int32), fps_numpy(P, 40)[0])


def covering_radius(P, chosen):
    """The largest distance from any point to its nearest chosen point (float64: a judgement, not a bit pattern)."""
    P = P.astype(np.float64)
    d = ((P[:, None, :] - P[None, chosen, :]) ** 2).sum(-1)
    return float(np.sqrt(d.min(1).max()))


def purpose_cloud():
    """A unit sphere of 4 000 points, 90 % of them in the cap z > 0.8, shuffled with a fixed seed."""
    rng = np.random.RandomState(31)

    def sphere(n, zlo, zhi):
        z, phi = rng.uniform(zlo, zhi, n), rng.uniform(0, 2 * np.pi, n)
        s = np.sqrt(1 - z * z)
        return np.stack([s * np.cos(phi), s * np.sin(phi), z], 1)

    P = np.concatenate([sphere(3600, 0.8, 1.0), sphere(400, -1.0, 0.8)]).astype(np.float32)
    return P[rng.permutation(4000)]


def test_the_samples_cover_an_uneven_cloud_better_than_a_prefix_or_a_random_choice(gpu):
    """On the CPU with the numpy restatement: FPS 0.213, the first 128 points 0.905, the random choices 0.892, 1.093
    and 1.085 — a factor of four; the test asserts the strict inequality only."""
    from parsenet_codebase_amd.sampling import farthest_point_sample
    P, m = purpose_cloud(), 128
    sample = farthest_point_sample(torch.from_numpy(P).to(gpu), m).cpu().numpy()
    assert same(sample.astype(np.int32), fps_numpy(P, m)[0])
    fps = covering_radius(P, sample)
    others = {"first %d" % m: covering_radius(P, np.arange(m))}
    for seed in (0, 1, 2):                                       # trainer._subsample: np.arange shuffled, first m
        np.random.seed(seed)
        sel = np.arange(P.shape[0])
        np.random.shuffle(sel)
        others["random, seed %d" % seed] = covering_radius(P, sel[:m])
    print("covering radius: fps %.4f, %s" % (fps, ", ".join("%s %.4f" % kv for kv in sorted(others.items()))))
    for name, value in others.items():
        assert fps < value, name


def test_reduce_cloud_and_lift(gpu):
    from parsenet_codebase_amd.sampling import farthest_point_sample, lift, reduce_cloud
    rng = np.random.RandomState(41)
    P = np.stack([_uniform(1300, 13), _uniform(1300, 14)])
    N = rng.normal(size=P.shape).astype(np.float32)
    L = rng.randint(0, 9, P.shape[:2])
    T, Nt, Lt = (torch.from_numpy(a).to(gpu) for a in (P, N, L))
    m = 60
    red, nrm, lab, owner = reduce_cloud(T, m, Nt, Lt)
    sample, owner2, _ = farthest_point_sample(T, m, return_owner=True)
    assert torch.equal(owner, owner2) and owner.dtype == torch.int64
    for c in range(2):
        assert torch.equal(red[c], T[c][sample[c]]) and torch.equal(nrm[c], Nt[c][sample[c]])
        assert torch.equal(lab[c], Lt[c][sample[c]])
        # the lifted labels are the labels of the brute-force nearest sample (first minimum)
        Q = P[c][sample[c].cpu().numpy()]
        dx, dy, dz = (P[c][:, None, a] - Q[None, :, a] for a in range(3))
        near = ((dx * dx + dy * dy) + dz * dz).argmin(1)
        assert np.array_equal(lift(lab, owner)[c].cpu().numpy(), L[c][sample[c].cpu().numpy()][near])
    assert torch.equal(lift(torch.arange(m, device=gpu).expand(2, m), owner), owner)
    # single and list layouts, a trailing shape
    r1, n1, o1 = reduce_cloud(T[0], m, Nt[0])
    assert torch.equal(r1, red[0]) and torch.equal(n1, nrm[0]) and torch.equal(o1, owner[0])
    assert torch.equal(lift(torch.arange(m, device=gpu), o1), o1)
    rl, nl, ol = reduce_cloud([T[0], T[1][:900]], m, [Nt[0], Nt[1][:900]], start=[0, 3])
    assert torch.equal(rl[0], red[0]) and torch.equal(nl[0], nrm[0]) and tuple(rl[1].shape) == (m, 3)
    member = torch.from_numpy(rng.uniform(size=(m, 4)).astype(np.float32)).to(gpu)
    assert torch.equal(lift([member, member], ol)[1], member[ol[1]])
    # the errors
    with pytest.raises(ValueError, match="cannot give m"):
        reduce_cloud([T[0], T[1][:30]], m)
    bad = T[0].clone()
    bad[5, 0] = float("nan")
    with pytest.raises(ValueError, match="owner holds -1"):
        lift(lab[0], farthest_point_sample(bad, m, return_owner=True)[1])
    with pytest.raises(ValueError, match="m must be"):
        farthest_point_sample(T, 0)
    for start in (1.5, "0", [0.0, 1.0], [0, 1, 2]):
        with pytest.raises(ValueError, match="start"):
            farthest_point_sample(T, m, start=start)
    with pytest.raises(TypeError, match="float32"):
        farthest_point_sample(T.double(), m)
    with pytest.raises(RuntimeError, match="MI355X only"):
        farthest_point_sample(T.cpu(), m)


def test_the_abi_on_the_gpu(gpu):
    from parsenet_codebase_amd import _lib
    lib = load_raw()
    assert [lib.pn_fps_launches(m) for m in (1, 7, 512)] == [3, 9, 514]
    P = torch.from_numpy(_uniform(2000, 15)).to(gpu)
    off = _off([2000], gpu)
    m = 7
    need = lib.pn_fps_workspace_bytes(2000, 1, m)
    ws = torch.zeros(need, dtype=torch.uint8, device=gpu)
    sample = torch.full((1, m), -7, dtype=torch.int32, device=gpu)
    real = dict(pts=P.data_ptr(), off=off.data_ptr(), S=1, total=2000, max_n=2000, m=m, sample=sample.data_ptr(),
                ws=ws.data_ptr(), ws_bytes=need)
    check_invalid_arguments(lib, **real)
    torch.cuda.synchronize()
    assert (sample == -7).all() and (ws == 0).all()              # refused calls launched nothing
    from tests.test_fps_abi import raw_call
    assert raw_call(lib, **dict(real, stream=_lib.current_stream(gpu))) == 0
    torch.cuda.synchronize()
    assert same(sample.cpu().numpy(), fps_numpy_batch([P.cpu().numpy()], m)[0])
