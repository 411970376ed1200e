"""GPU checks of the rigid registration (csrc/register.hip) against ``register_numpy``, the numpy restatement of
tests/test_register_abi.py: every output of the kernels equal bit for bit on every case of that file, in both modes; the
move step as a call of its own; the public functions in the three layouts; independence of the developer hook, of the
run and of the batch; a merged pair of scans."""
import os

import numpy as np
import pytest
import torch

from tests.test_fps_abi import same
from tests.test_register_abi import (CASES, CONVERGED, JITTER, PYRAMID, apply_numpy, cases, equal, flat_case, motion,
                                     pyramid_pair, reference_of, scan, torus_pair, which_differ)

pytestmark = pytest.mark.gpu
DEV = "cuda"


def gpu_register(c, want_pairs=True):
    from parsenet_codebase_amd import kernels
    S, src, off_s, tgt, off_t, nrm, init = flat_case(c)
    t = lambda a: None if a is None else torch.from_numpy(a).to(DEV)      # noqa: E731
    out = kernels.register_ragged(t(src), t(off_s), t(tgt), t(off_t), c["max_dist"], c["mode"], t(nrm),
                                  None if init is None else t(init).reshape(S, 4, 4), c["max_iter"], c["tol"][0],
                                  c["tol"][1], want_pairs=want_pairs)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy().reshape(S, 16) if k == 0 else o.cpu().numpy() for k, o in enumerate(out))


@pytest.mark.parametrize("name", CASES)
def test_the_kernels_equal_the_definition(name):
    got, want = gpu_register(cases()[name]), reference_of(name)
    assert equal(got, want), (name, which_differ(got, want))


def test_the_outputs_without_pairs_and_two_calls_give_the_same_bits():
    c = cases()["torus, plane"]
    a, b = gpu_register(c), gpu_register(c)
    assert equal(a, b) and equal(gpu_register(c, want_pairs=False), a[:5])


def test_the_results_do_not_depend_on_the_binning_hook():
    names = ("partial overlap", "tile edges batch, plane")
    old = os.environ.get("PN_KNN3_QUERY_BIN")
    try:
        os.environ["PN_KNN3_QUERY_BIN"] = "0"
        got = [gpu_register(cases()[n]) for n in names]
    finally:
        if old is None:
            del os.environ["PN_KNN3_QUERY_BIN"]
        else:
            os.environ["PN_KNN3_QUERY_BIN"] = old
    for n, g in zip(names, got):
        assert equal(g, reference_of(n)), (n, which_differ(g, reference_of(n)))


def test_rigid_apply_is_the_move_step():
    from parsenet_codebase_amd import kernels
    P = [scan(n, 30 + n)[0] for n in (0, 1, 1025, 300)]
    Ms = [motion(33.0), motion(180.0, (0, 0, 1)), motion(179.0, (1, 0, 0)), np.eye(4)]
    off = torch.from_numpy(np.concatenate([[0], np.cumsum([p.shape[0] for p in P])]).astype(np.int32)).to(DEV)
    out = kernels.rigid_apply(torch.from_numpy(np.concatenate(P)).to(DEV), off, torch.from_numpy(np.stack(Ms)).to(DEV))
    assert same(out.cpu().numpy(), np.concatenate([apply_numpy(p, M) for p, M in zip(P, Ms)]))


def test_register_in_the_three_layouts_and_apply_transform():
    from parsenet_codebase_amd.registration import STATUS_NAMES, apply_transform, register
    src, tgt, nrm, perm = torus_pair()
    want = reference_of("torus, plane")
    s, t, n = (torch.from_numpy(a).to(DEV) for a in (src, tgt, nrm))
    T, info = register(s, t, float("inf"), method="plane", target_normals=n, max_iter=30, return_info=True)
    assert tuple(T.shape) == (4, 4) and same(T.cpu().numpy().reshape(16), want[0][0])
    assert info["status"].dim() == 0 and STATUS_NAMES[int(info["status"])] == "converged" == STATUS_NAMES[CONVERGED]
    assert int(info["iterations"]) == want[1][0] and int(info["count"]) == 1500 and float(info["rmse"]) == want[4][0]
    assert info["idx"].dtype == torch.int64 and np.array_equal(info["idx"].cpu().numpy(), perm)
    assert same(info["dist"].cpu().numpy(), want[6])
    Tb = register(torch.stack([s, s]), torch.stack([t, t]), float("inf"), method="plane",
                  target_normals=torch.stack([n, n]), max_iter=30)
    assert tuple(Tb.shape) == (2, 4, 4) and same(Tb[0].cpu().numpy(), T.cpu().numpy()) and torch.equal(Tb[0], Tb[1])
    point = reference_of("torus, point")
    Tl, il = register([s, s[:400]], [t, t], float("inf"), max_iter=30, return_info=True,
                      init=torch.eye(4, dtype=torch.float64))
    assert tuple(Tl.shape) == (2, 4, 4) and same(Tl[0].cpu().numpy().reshape(16), point[0][0])
    assert isinstance(il["idx"], list) and [tuple(v.shape) for v in il["idx"]] == [(1500,), (400,)]
    assert il["status"].tolist() == [CONVERGED, CONVERGED] and np.array_equal(il["idx"][1].cpu().numpy(), perm[:400])
    # apply_transform: the points by the move step, the normals rotated only
    M = T.cpu().numpy()
    back, rot = apply_transform(s, T, s)
    assert same(back.cpu().numpy(), apply_numpy(src, M))
    R = M.copy()
    R[:3, 3] = 0.0
    assert same(rot.cpu().numpy(), apply_numpy(src, R))
    assert np.abs(back.cpu().numpy() - tgt[perm]).max() <= 4 * 2.0 ** -24 * 2.0                 # it lands on the target
    lb = apply_transform([s, s[:7]], Tl)
    assert isinstance(lb, list) and same(lb[1].cpu().numpy(), apply_numpy(src[:7], Tl[1].cpu().numpy()))


def test_a_merged_pair_has_the_voxels_of_the_target():
    """The recipe of the README: register, apply, concatenate, downsample.  The source is the target moved, so at a voxel
    of ten jitters the merged cloud occupies the cells the target occupies... exactly when the registration is right: a
    misaligned copy would add cells along the whole surface."""
    from parsenet_codebase_amd.registration import apply_transform, register
    from parsenet_codebase_amd.sampling import voxel_downsample
    src, tgt, nrm, _ = torus_pair()
    s, t, n = (torch.from_numpy(a).to(DEV) for a in (src, tgt, nrm))
    T = register(s, t, 0.3, method="plane", target_normals=n, max_iter=30)
    voxel = 10 * JITTER
    origin = tuple(float(v) for v in (tgt.min(0) - np.float32(0.5 * voxel)))
    alone = voxel_downsample(t, voxel, origin=origin)[0]
    merged = voxel_downsample(torch.cat([apply_transform(s, T), t]), voxel, origin=origin)[0]
    unaligned = voxel_downsample(torch.cat([s, t]), voxel, origin=origin)[0]
    assert merged.shape[0] == alone.shape[0] < unaligned.shape[0]


def test_the_pyramid_reaches_the_true_pairs_where_one_level_does_not():
    """From PYRAMID's start (40 degrees: tests/test_register_abi.py holds both halves on the restatement, and says why
    not 15) the pyramid's transform pairs every source point with its true target point; ``register`` alone with the
    last level's max_dist does not."""
    from parsenet_codebase_amd.neighbors import nearest
    from parsenet_codebase_amd.registration import apply_transform, register, register_pyramid
    src, tgt, perm = pyramid_pair()
    s, t = torch.from_numpy(src).to(DEV), torch.from_numpy(tgt).to(DEV)
    T = register_pyramid(s, t, PYRAMID["voxels"], PYRAMID["factor"], max_iter=PYRAMID["max_iter"])
    assert tuple(T.shape) == (4, 4) and np.array_equal(nearest(apply_transform(s, T), t)[:, 0].cpu().numpy(), perm)
    assert np.abs(T.cpu().numpy() @ motion(PYRAMID["angle"]) - np.eye(4)).max() <= 1e-3
    one = register(s, t, PYRAMID["factor"] * PYRAMID["voxels"][-1], max_iter=PYRAMID["max_iter"])
    assert not np.array_equal(nearest(apply_transform(s, one), t)[:, 0].cpu().numpy(), perm)
    Tl, info = register_pyramid([s], [t], PYRAMID["voxels"], PYRAMID["factor"], max_iter=PYRAMID["max_iter"],
                                return_info=True)
    assert torch.equal(Tl[0], T) and info["status"].tolist() == [CONVERGED] and isinstance(info["idx"], list)
