"""GPU checks of the dominant-plane extraction (csrc/plane.hip, parsenet_codebase_amd/cleaning.py): plane, count, best,
inlier and dist equal to the numpy restatement of the definition (tests.test_plane_abi.plane_numpy) bit for bit on the
clouds and the ragged batches of the CPU tests, on a second run, alone and in a batch; fit_plane in its three layouts,
remove_plane and peel_planes with gathered per-point arrays, their errors, and the scene the feature exists for: parts
above a table, which the clusters cannot tell apart until the table is gone.  Every comparison is exact: there is no
tolerance in this file."""
import numpy as np
import pytest
import torch

from tests.test_cluster_abi import cluster_numpy
from tests.test_plane_abi import (CASES, OUTPUTS, TABLETOP, cases, check_properties, equal, min_cos_of, one,
                                  perpendicular_planes, plane_and_sphere, plane_numpy, plane_numpy_batch,
                                  ragged_batches, same, tabletop_scene, unit_axis)

pytestmark = pytest.mark.gpu


def _off(sizes, gpu):
    return torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)).to(gpu)


def _plane(gpu, clouds, thresholds, H, seed, refine, axis=None, max_angle=None, as_clouds=False):
    """kernels.plane_ragged on a ragged batch of numpy clouds -> (plane, count, best, inlier, dist) as numpy."""
    from parsenet_codebase_amd import kernels as K
    from parsenet_codebase_amd.ragged import Clouds
    t = torch.from_numpy(np.asarray(thresholds, np.float32)).to(gpu)
    if as_clouds:
        off = Clouds([torch.from_numpy(np.ascontiguousarray(c, np.float32).reshape(-1, 3)).to(gpu) for c in clouds], "test")
        flat = off.flat
    else:
        flat = torch.from_numpy(np.concatenate([c.reshape(-1, 3) for c in clouds]).astype(np.float32)).to(gpu)
        off = _off([c.shape[0] for c in clouds], gpu)
    out = K.plane_ragged(flat, off, t, H, seed, refine, axis, max_angle)
    return tuple(o.cpu().numpy().astype(np.uint8) if o.dtype == torch.bool else o.cpu().numpy() for o in out)


def _check(gpu, clouds, thresholds, H, seed, refine, axis, max_angle, what, want):
    got = _plane(gpu, clouds, thresholds, H, seed, refine, axis, max_angle)
    for name, g, w in zip(OUTPUTS, got, want):
        assert same(g, np.asarray(w, g.dtype)), "%s: %s differs" % (what, name)
    again = _plane(gpu, clouds, thresholds, H, seed, refine, axis, max_angle, as_clouds=True)
    assert all(same(a, b) for a, b in zip(got, again)), "%s: a second run changed a result" % what
    return got


def _user_axis(c):
    """(axis, max_angle) that give the case's unit axis and min_cos."""
    if c["axis"] is None:
        return None, None
    for angle in (0, 10, 30):
        if c["min_cos"] == min_cos_of(angle):
            return tuple(c["axis"].tolist()), angle
    raise AssertionError("a case with an angle this file does not know")


@pytest.fixture(scope="module")
def reference():
    """name -> plane_numpy of the case: computed once, shared, never changed."""
    return {name: plane_numpy(c["cloud"], c["t"], c["H"], c["seed"], c["refine"], c["axis"], c["min_cos"])
            for name, c in cases().items()}


@pytest.mark.parametrize("name", CASES)
def test_the_kernels_equal_the_definition(gpu, reference, name):
    c, want = cases()[name], reference[name]
    axis, angle = _user_axis(c)
    if axis is not None:                                 # the unit axis survives the host's normalisation bit for bit
        assert same(unit_axis(axis), c["axis"])
    got = _check(gpu, [c["cloud"]], [c["t"]], c["H"], c["seed"], c["refine"], axis, angle, name, one(want))
    assert got[2][0] == want["best"]
    if name in EXPECT_A_PLANE:
        assert got[2][0] >= 0 and got[1][0] >= 3, name    # a case that expects a plane must find one
    check_properties(c, dict(want, plane=got[0][0], count=int(got[1][0]), best=int(got[2][0]), inlier=got[3],
                             dist=got[4]))


EXPECT_A_PLANE = tuple(n for n in CASES if n not in (
    "collinear", "coincident", "planar, axis excludes everything", "plane and sphere 0", "plane and sphere 1",
    "plane and sphere 2"))


def test_the_case_list_is_the_one_of_the_cpu_tests():
    assert list(CASES) == sorted(cases()) and len(EXPECT_A_PLANE) == len(CASES) - 6


@pytest.mark.parametrize("name", ("empty first, middle and last", "non-finite clouds among clean ones",
                                  "thresholds that are none"))
def test_a_ragged_batch_alone_and_in_the_batch(gpu, name):
    clouds, ts, H, seed, refine, axis, min_cos = ragged_batches()[name]
    user = (None, None) if axis is None else (tuple(axis.tolist()), 40)
    assert axis is None or min_cos == min_cos_of(40)
    want = plane_numpy_batch(clouds, ts, H, seed, refine, axis, min_cos)
    got = _check(gpu, clouds, ts, H, seed, refine, user[0], user[1], name, want)
    o = 0
    for c, P in enumerate(clouds):                                           # every cloud alone gives what it gives here
        alone = _plane(gpu, [P], [ts[c]], H, seed, refine, *user)
        n = P.shape[0]
        assert equal(alone, (got[0][c:c + 1], got[1][c:c + 1], got[2][c:c + 1], got[3][o:o + n], got[4][o:o + n])), c
        o += n
    back = _plane(gpu, clouds[::-1], ts[::-1], H, seed, refine, *user)
    assert equal(back[:3], [g[::-1] for g in got[:3]])
    empty = np.zeros((0, 3), np.float32)
    _check(gpu, [empty, empty], [0.5, 0.0], 8, 1, 1, None, None, "empty clouds only",
           plane_numpy_batch([empty, empty], [0.5, 0.0], 8, 1, 1))


def _t(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def test_fit_plane_in_the_three_layouts(gpu):
    from parsenet_codebase_amd.cleaning import fit_plane
    A, B, C = plane_and_sphere(700, 41), plane_and_sphere(700, 42), plane_and_sphere(300, 43)
    args = dict(hypotheses=64, seed=5, refine=2)
    wa, wb, wc = (plane_numpy(P, t, 64, 5, 2) for P, t in ((A, 0.02), (B, 0.02), (C, 0.03)))
    assert min(w["best"] for w in (wa, wb, wc)) >= 0
    plane, inlier = fit_plane(_t(A, gpu), 0.02, **args)                                   # one cloud
    assert plane.shape == (4,) and plane.dtype == torch.float64 and inlier.dtype == torch.bool and inlier.shape == (700,)
    assert same(plane.cpu().numpy(), wa["plane"]) and same(inlier.cpu().numpy().astype(np.uint8), wa["inlier"])
    plane, inlier, count, best, dist = fit_plane(_t(A, gpu), 0.02, return_info=True, **args)
    assert count.shape == () and int(count) == wa["count"] and int(best) == wa["best"]
    assert same(dist.cpu().numpy(), wa["dist"]) and same(plane.cpu().numpy(), wa["plane"])
    plane, inlier, count, best, dist = fit_plane(_t(np.stack([A, B]), gpu), 0.02, return_info=True, **args)   # a batch
    assert plane.shape == (2, 4) and inlier.shape == (2, 700) and dist.shape == (2, 700) and count.shape == (2,)
    for b, w in enumerate((wa, wb)):
        assert same(plane[b].cpu().numpy(), w["plane"]) and same(dist[b].cpu().numpy(), w["dist"])
        assert same(inlier[b].cpu().numpy().astype(np.uint8), w["inlier"])
        assert int(count[b]) == w["count"] and int(best[b]) == w["best"]
    plane, inlier, count, best, dist = fit_plane([_t(A, gpu), _t(C, gpu)], [0.02, 0.03], return_info=True, **args)
    assert all(isinstance(v, list) and len(v) == 2 for v in (plane, inlier, count, best, dist))          # a list
    for b, w in enumerate((wa, wc)):
        assert same(plane[b].cpu().numpy(), w["plane"]) and same(dist[b].cpu().numpy(), w["dist"])
        assert same(inlier[b].cpu().numpy().astype(np.uint8), w["inlier"])
        assert int(count[b]) == w["count"] and int(best[b]) == w["best"]
    plane, inlier = fit_plane(_t(A, gpu), 0.02, axis=(0, 0, 3), max_angle=30, **args)                    # an axis
    w = plane_numpy(A, 0.02, 64, 5, 2, unit_axis((0, 0, 3)), min_cos_of(30))
    assert w["best"] >= 0 and same(plane.cpu().numpy(), w["plane"])
    assert same(inlier.cpu().numpy().astype(np.uint8), w["inlier"])


def test_remove_plane_hands_out_the_rest_or_the_plane(gpu):
    from parsenet_codebase_amd.cleaning import remove_plane, restore
    A, C = plane_and_sphere(700, 41), plane_and_sphere(300, 43)
    bad = plane_and_sphere(100, 44)
    bad[5, 0] = np.nan
    args = dict(hypotheses=64, seed=5, refine=2)
    wa, wc = plane_numpy(A, 0.02, 64, 5, 2), plane_numpy(C, 0.03, 64, 5, 2)
    colour = np.arange(700 * 2, dtype=np.int16).reshape(700, 2)
    for keep, mask in (("rest", wa["inlier"] == 0), ("plane", wa["inlier"] == 1)):
        pts, col, index, plane = remove_plane(_t(A, gpu), _t(colour, gpu), threshold=0.02, keep=keep, **args)
        want = np.flatnonzero(mask)
        assert index.dtype == torch.int64 and same(index.cpu().numpy(), want) and (np.diff(want) > 0).all()
        assert same(pts.cpu().numpy(), A[want]) and col.dtype == torch.int16 and same(col.cpu().numpy(), colour[want])
        assert same(plane.cpu().numpy(), wa["plane"])
        back = restore(col, index, 700, -1).cpu().numpy()                        # the round trip
        assert same(back[want], colour[want]) and (np.delete(back, want, 0) == -1).all()
    tags = [np.arange(700, dtype=np.int64), np.arange(300, dtype=np.int64) + 1000, np.arange(100, dtype=np.int64)]
    for keep in ("rest", "plane"):
        pts, tag, index, plane = remove_plane([_t(A, gpu), _t(C, gpu), _t(bad, gpu)], [_t(v, gpu) for v in tags],
                                              threshold=[0.02, 0.03, 0.02], keep=keep, **args)
        for b, (P, w) in enumerate(((A, wa), (C, wc))):
            want = np.flatnonzero(w["inlier"] == (keep == "plane"))
            assert same(index[b].cpu().numpy(), want) and same(pts[b].cpu().numpy(), P[want])
            assert same(tag[b].cpu().numpy(), tags[b][want]) and same(plane[b].cpu().numpy(), w["plane"])
        # a cloud with a non-finite coordinate has no plane: all of it under "rest", nothing under "plane"
        assert index[2].shape[0] == (100 if keep == "rest" else 0) and not plane[2].cpu().numpy().any()
        assert same(index[2].cpu().numpy(), np.arange(100 if keep == "rest" else 0))


def test_peel_planes_finds_the_planes_in_order_of_size(gpu):
    from parsenet_codebase_amd.cleaning import peel_planes
    rng = np.random.RandomState(51)
    walls, on_floor = perpendicular_planes(1500, 52)
    ball = rng.normal(size=(300, 3))
    ball = 0.3 * ball / np.linalg.norm(ball, axis=1, keepdims=True) + np.asarray([-0.2, 0.1, 0.6])
    P = np.concatenate([walls, ball.astype(np.float32)])
    truth = np.concatenate([np.where(on_floor, 0, 1), np.full(300, 2)])
    order = rng.permutation(1800)
    P, truth = P[order], truth[order]
    tag = np.arange(1800, dtype=np.int32)
    planes, rest = peel_planes(_t(P, gpu), _t(tag, gpu), threshold=0.012, max_planes=4, min_inliers=200,
                               hypotheses=128, seed=7)
    assert len(planes) == 2                                          # the ball holds no plane of 200 points: it stops
    seen = []
    for p, (pts, tg, index, plane) in enumerate(planes):
        index = index.cpu().numpy()
        assert index.dtype == np.int64 and (np.diff(index) > 0).all()                      # original rows, ascending
        assert same(pts.cpu().numpy(), P[index]) and same(tg.cpu().numpy(), tag[index])
        assert (truth[index] == p).mean() > 0.97 and (truth == p).sum() * 0.97 < index.shape[0]   # floor, then wall
        assert abs(float(plane[2 if p == 0 else 0])) > 0.99
        seen.append(index)
    assert seen[0].shape[0] > seen[1].shape[0]
    pts, tg, index = rest
    seen.append(index.cpu().numpy())
    assert same(pts.cpu().numpy(), P[seen[2]]) and same(tg.cpu().numpy(), tag[seen[2]])
    assert same(np.sort(np.concatenate(seen)), np.arange(1800, dtype=np.int64))            # disjoint, and together all
    # round p uses seed + p on what round p - 1 left
    first = plane_numpy(P, 0.012, 128, 7, 1)
    assert same(seen[0], np.flatnonzero(first["inlier"]))
    left = np.flatnonzero(first["inlier"] == 0)
    second = plane_numpy(P[left], 0.012, 128, 8, 1)
    assert same(seen[1], left[np.flatnonzero(second["inlier"])])
    planes, rest = peel_planes(_t(P, gpu), threshold=0.012, max_planes=1, min_inliers=200, hypotheses=128, seed=7)
    assert len(planes) == 1 and rest[0].shape[0] == 1800 - seen[0].shape[0]
    planes, rest = peel_planes(_t(P, gpu), threshold=0.012, max_planes=4, min_inliers=1700, hypotheses=128, seed=7)
    assert planes == [] and same(rest[1].cpu().numpy(), np.arange(1800, dtype=np.int64))


def test_argument_errors_come_before_any_launch(gpu):
    from parsenet_codebase_amd import cleaning, kernels
    P = torch.zeros(8, 3, device=gpu)
    off = torch.tensor([0, 8], dtype=torch.int32, device=gpu)
    t = torch.full((1,), 0.1, device=gpu)
    for H in (0, 4097, 1.5, True):
        with pytest.raises(ValueError, match="hypotheses must be"):
            kernels.plane_ragged(P, off, t, hypotheses=H)
        with pytest.raises(ValueError, match="hypotheses must be"):
            cleaning.fit_plane(P, 0.1, hypotheses=H)
    for refine in (-1, 5):
        with pytest.raises(ValueError, match="refine must be"):
            kernels.plane_ragged(P, off, t, refine=refine)
        with pytest.raises(ValueError, match="refine must be"):
            cleaning.remove_plane(P, threshold=0.1, refine=refine)
    for axis, angle in (((0, 0, 1), None), (None, 10)):
        with pytest.raises(ValueError, match="axis and max_angle come together"):
            cleaning.fit_plane(P, 0.1, axis=axis, max_angle=angle)
    with pytest.raises(ValueError, match="axis must be finite and not zero"):
        cleaning.fit_plane(P, 0.1, axis=(0, 0, 0), max_angle=10)
    with pytest.raises(ValueError, match="max_angle must be"):
        cleaning.fit_plane(P, 0.1, axis=(0, 0, 1), max_angle=91)
    with pytest.raises(ValueError, match=r"threshold must be \(1,\)"):
        kernels.plane_ragged(P, off, torch.full((2,), 0.1, device=gpu))
    with pytest.raises(TypeError, match="must be on the GPU"):
        kernels.plane_ragged(P.cpu(), off, t)
    with pytest.raises(TypeError, match="must be on the GPU"):
        kernels.plane_ragged(P, off, t.cpu())
    with pytest.raises(TypeError, match="float32"):
        kernels.plane_ragged(P.double(), off, t)
    with pytest.raises(TypeError, match="float32"):
        cleaning.fit_plane(P.double(), 0.1)
    with pytest.raises(ValueError, match='keep must be "rest" or "plane"'):
        cleaning.remove_plane(P, threshold=0.1, keep="both")


def test_the_table_links_the_parts_until_it_is_taken_out(gpu):
    """The reason for the feature.  6 000 points: 60 % on the table z = 0 with a jitter within t / 2, two tori floating
    4.5 t above it and further from each other than the cluster radius.  The clusters see ONE object; without the table
    they see exactly the two tori.  Conditions, not tolerances: every table point is within t / 2 of the truth and every
    other point at least 4 t away, so they fail only if the plane found is wrong."""
    from parsenet_codebase_amd.cleaning import remove_plane, split_clusters
    P, part = tabletop_scene()
    t, r = TABLETOP["t"], TABLETOP["radius"]
    want = plane_numpy(P, t, 512, 0, 1, unit_axis((0, 0, 1)), min_cos_of(10))
    assert same(want["inlier"], (part == 0).astype(np.uint8))                       # plane_numpy == the truth
    scene = _t(P, gpu)
    got = _check(gpu, [P], [t], 512, 0, 1, (0, 0, 1), 10, "tabletop", one(want))    # plane_ragged == plane_numpy
    assert got[2][0] >= 0 and same(got[3], (part == 0).astype(np.uint8))
    whole = split_clusters(scene, radius=r)
    assert len(whole) == 1 and whole[0][0].shape[0] == 6000 and cluster_numpy(P, r)[1] == 1
    pts, index, plane = remove_plane(scene, threshold=t, axis=(0, 0, 1), max_angle=10)
    assert same(index.cpu().numpy(), np.flatnonzero(part != 0)) and same(plane.cpu().numpy(), want["plane"])
    objects = split_clusters(pts, radius=r)
    assert len(objects) == 2
    found = sorted(index.cpu().numpy()[o[1].cpu().numpy()].tolist() for o in objects)
    assert found == sorted(np.flatnonzero(part == k).tolist() for k in (1, 2))
