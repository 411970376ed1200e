"""GPU: the Epanechnikov kernel below ``MeanShift.mean_shift`` — the forward-only state, the centre-rows backward
(the Epanechnikov instantiation of csrc/meanshift_rows.hip) and the stages built on them.

The kernel's derivative jumps at the edge of its support, so every input of the row tests is tight clusters on
the unit sphere: inside a cluster every pair is well inside the support, across clusters well outside, and the
tests first CHECK in float64 that no pair of (row of any iterate, data point) lies within 1e-3 of the edge
(``_oracle``: all N rows, no pair skipped).  Bars: those of tests/test_meanshift_epa_gpu.py for the dense
Epanechnikov passes against the same oracle — rows 1e-5, gradient 5e-5 of its largest entry."""
import numpy as np
import pytest
import torch

from tests.test_meanshift_epa_gpu import GRAD_BAR, ITER_BAR
from tests.test_meanshift_gpu import _canonical, _clustered, _rel

pytestmark = pytest.mark.gpu

B, N, T, C = 2, 300, 3, 4            # N: four full 64-point blocks and a ragged one of 44
BWS = (0.4, 0.5)
SPREAD = 0.15
EDGE = 1e-3
WIDTHS = (32, 64, 128)
_CACHE = {}


def _inputs(D):
    """X (B,N,D) unit rows in C tight clusters per item and their labels (B,N)."""
    Xs, labs = zip(*[_clustered(N, C, 700 + D + i, spread=SPREAD, d=D) for i in range(B)])
    return torch.stack(Xs), torch.stack(labs)


def _ids(lab, R, avoid=None):
    """(B,R) row ids, one id repeated inside every item; ``avoid``: no row of that cluster in item 0."""
    g = torch.Generator().manual_seed(R)
    ids = torch.randint(0, N, (B, R), generator=g)
    if avoid is not None:
        ok = torch.nonzero(lab[0] != avoid).flatten()
        ids[0] = ok[torch.randint(0, ok.numel(), (R,), generator=g)]
    ids[:, R - 1] = ids[:, R - 2]
    return ids


def _iterates64(X, b):
    """The reference's loop (src/mean_shift.py:45-79 with the Epanechnikov form of kernel_between, :64-68) in float64
    on one item: the list of the T + 1 iterates, with autograd, and the smallest | 1 - dist / b^2 | over all pairs
    (row of an iterate that a step reads, data point)."""
    x = X.double().requires_grad_(True)
    its, edge = [x], float("inf")
    for _ in range(T):
        with torch.no_grad():
            edge = min(edge, float((1 - (2.0 - 2.0 * its[-1] @ x.t()) / b ** 2).abs().min()))
        its.append(_step64(its[-1], x, b))
    return x, its, edge


def _step64(q, x, b):
    """One pass of the loop of src/mean_shift.py:45-79 with kernel_between's Epanechnikov form (:64-68)."""
    Kmat = torch.nn.functional.relu(3 / 4 * (1 - (2.0 - 2.0 * q @ x.t()) / (b ** 2)))
    D_ = 1 / torch.sum(Kmat, 1, keepdim=True)
    q = q + ((Kmat @ x) * D_ - q)
    return q / torch.norm(q, dim=1, p=2, keepdim=True)


def _oracle(D, R, avoid=None):
    """float64 rows and gradient of sum(rows * w) for the inputs of width D and R ids (computed once per case):
    (X, lab, ids, w, rows64 (B,R,D), grad64 (B,N,D), iterates (B x [T + 1 x (N,D)]), edge)."""
    key = (D, R, avoid)
    if key not in _CACHE:
        X, lab = _inputs(D)
        ids = _ids(lab, R, avoid)
        w = torch.randn(B, R, D, generator=torch.Generator().manual_seed(5 + R))
        rows, grads, iterates, edge = [], [], [], float("inf")
        for i in range(B):
            x, its, e = _iterates64(X[i], BWS[i])
            r = its[-1][ids[i]]
            (r * w[i].double()).sum().backward()
            rows.append(r.detach())
            grads.append(x.grad)
            iterates.append([t.detach() for t in its])
            edge = min(edge, e)
        _CACHE[key] = (X, lab, ids, w, torch.stack(rows), torch.stack(grads), iterates, edge)
    return _CACHE[key]


def _rows_run(gpu, X, ids, w):
    from parsenet_codebase_amd import mean_shift as MSM
    xg = X.to(gpu).requires_grad_(True)
    new_X, state = MSM.mean_shift_iterations_state(xg, torch.tensor(BWS, device=gpu), T, kernel_type="epa")
    c = MSM.centre_rows(xg, state, ids.to(gpu))
    (c * w.to(gpu)).sum().backward()
    return new_X, state, c.detach(), xg.grad


@pytest.mark.parametrize("R", [5, 64])
@pytest.mark.parametrize("D", WIDTHS)
def test_centre_rows_against_fp64(gpu, D, R):
    """1. Rows of the final iterate and d sum(rows * w) / dX from the Epanechnikov state + centre_rows against the
    float64 oracle; no pair within 1e-3 of the edge of the support in any iterate (checked, not assumed); every row
    has points on its support (its cluster) and off it (the other clusters).  Also: the call is a fused Epanechnikov
    one and leaves the Gaussian calls' bookkeeping alone."""
    from parsenet_codebase_amd import kernels as K, mean_shift as MSM
    X, lab, ids, w, rows64, grad64, iterates, edge = _oracle(D, R)
    print("width %d: smallest |1 - dist / b^2| over all pairs and iterates %.3e" % (D, edge))
    assert edge > EDGE
    for i in range(B):
        on = (2.0 - 2.0 * iterates[i][0] @ iterates[i][0].t()) < BWS[i] ** 2
        assert bool(on.any(1).all()) and bool((~on).any(1).all())
    before, others = MSM.CALLS_EPA, (dict(MSM.CALLS), MSM.CALLS_W, dict(MSM._AUTO))
    new_X, state, c, grad = _rows_run(gpu, X, ids, w)
    assert MSM.CALLS_EPA == before + 1 and (dict(MSM.CALLS), MSM.CALLS_W, dict(MSM._AUTO)) == others
    assert state.kind == K.KERNEL_EPANECHNIKOV and state.inv is None and not new_X.requires_grad
    assert torch.equal(c, torch.gather(new_X, 1, ids.to(gpu).unsqueeze(2).expand(-1, -1, D)))
    for i in range(B):
        er, eg = _rel(c[i], rows64[i]), _rel(grad[i], grad64[i])
        print("epa rows against fp64, width %d, R %d, item %d (b %.2f): rows %.2e gradient %.2e"
              % (D, R, i, BWS[i], er, eg))
        assert er < ITER_BAR
        assert eg < GRAD_BAR


@pytest.mark.parametrize("R", [5, 64])
@pytest.mark.parametrize("D", WIDTHS)
def test_centre_rows_against_the_dense_backward(gpu, D, R):
    """2. The same rows and gradient against ``mean_shift_iterations(kernel_type="epa")`` gathered at the ids and
    back-propagated through the dense passes, same bars; and a repeated id accumulates: the gradient of (ids with
    the last one repeated, w) is that of (ids without the repeat, the two weights added)."""
    from parsenet_codebase_amd import mean_shift as MSM
    X, lab, ids, w = _oracle(D, R)[:4]
    idg, wg = ids.to(gpu), w.to(gpu)
    xd = X.to(gpu).requires_grad_(True)
    yd = MSM.mean_shift_iterations(xd, torch.tensor(BWS, device=gpu), T, kernel_type="epa")
    cd = torch.gather(yd, 1, idg.unsqueeze(2).expand(-1, -1, D))
    (cd * wg).sum().backward()
    _, _, c, grad = _rows_run(gpu, X, ids, w)
    w_sum = w[:, :R - 1].clone()
    w_sum[:, R - 2] += w[:, R - 1]
    grad_sum = _rows_run(gpu, X, ids[:, :R - 1].contiguous(), w_sum)[3]
    for i in range(B):
        er, eg, ea = _rel(c[i], cd[i]), _rel(grad[i], xd.grad[i]), _rel(grad[i], grad_sum[i])
        print("epa rows against dense, width %d, R %d, item %d: rows %.2e gradient %.2e repeated id %.2e"
              % (D, R, i, er, eg, ea))
        assert er < ITER_BAR
        assert eg < GRAD_BAR
        assert ea < GRAD_BAR


@pytest.mark.parametrize("D", WIDTHS)
def test_gaussian_profile_is_the_old_entry_point_bit_for_bit(gpu, D):
    """3. ``K.meanshift_rows_bwd(kind=KERNEL_GAUSSIAN)`` (pn_meanshift_rows_bwd_kind_f32) and
    pn_meanshift_rows_bwd_f32 on one step of a Gaussian state: gq and gx equal bit for bit."""
    from parsenet_codebase_amd import _lib, kernels as K, mean_shift as MSM
    from parsenet_codebase_amd.kernels import current_stream, ptr
    torch.cuda.set_device(gpu)
    R = 40
    X, lab = _inputs(D)
    ids = _ids(lab, R).to(gpu)
    x = X.to(gpu)
    bw = torch.tensor(BWS, device=gpu) * 0.5
    _, state = MSM.mean_shift_iterations_state(x, bw, 1)
    assert state.inv is None and state.kind == K.KERNEL_GAUSSIAN
    take = lambda t: torch.gather(t, 1, ids.unsqueeze(2).expand(-1, -1, D)).contiguous()
    q, y = take(state.iterates[0]), take(state.iterates[1])
    rs, un = torch.gather(state.rsums[0], 1, ids).contiguous(), torch.gather(state.norms[0], 1, ids).contiguous()
    gy = torch.randn(B, R, D, generator=torch.Generator().manual_seed(D)).to(gpu)
    seed = torch.randn(B, N, D, generator=torch.Generator().manual_seed(D + 1)).to(gpu)   # (the kernel ADDS into gx)
    gx_new = seed.clone()
    gq_new = K.meanshift_rows_bwd(gy, y, q, rs, un, state.x, state.bsq, gx_new, kind=K.KERNEL_GAUSSIAN)
    gx_old, gq_old = seed.clone(), torch.empty_like(q)
    ws = K.meanshift_rows_workspace(B, N, x.device)
    with _lib.on_device(x.device):
        rc = _lib.load().pn_meanshift_rows_bwd_f32(ptr(gy), ptr(y), ptr(q), ptr(rs), ptr(un), ptr(state.x),
                                                   ptr(state.bsq), B, N, D, R, ptr(gq_old), ptr(gx_old), ptr(ws),
                                                   ws.numel(), current_stream(x.device))
    assert rc == 0
    assert torch.equal(gq_new, gq_old) and torch.equal(gx_new, gx_old)
    assert bool(torch.isfinite(gq_new).all()) and float(gq_new.abs().max()) > 0 and not torch.equal(gx_new, seed)


@pytest.mark.parametrize("D", WIDTHS)
def test_off_support_gradient_is_exactly_zero(gpu, D):
    """4. No selected row of item 0 comes from cluster 3, and — checked in float64 on every iterate — every point of
    that cluster is off the support of every selected row in every step: its rows of X.grad are 0.0 exactly (gs is
    a select, K / r a product with an exact zero; nothing is added to those rows), while the selected clusters'
    rows are not."""
    R, far = 5, 3
    X, lab, ids, w, rows64, grad64, iterates, edge = _oracle(D, R, avoid=far)
    assert edge > EDGE
    members = lab[0] == far
    assert int(members.sum()) > 40 and not bool(members[ids[0]].any())
    data = iterates[0][0]
    for it in iterates[0][:T]:
        assert bool(((2.0 - 2.0 * it[ids[0]] @ data[members].t()) > BWS[0] ** 2).all())
    assert float(grad64[0][members].abs().max()) == 0.0
    grad = _rows_run(gpu, X, ids, w)[3]
    assert bool((grad[0][members.to(gpu)] == 0.0).all())
    assert float(grad[0][~members.to(gpu)].abs().max()) > 0
    assert _rel(grad[0], grad64[0]) < GRAD_BAR


@pytest.mark.parametrize("D", WIDTHS)
def test_two_backward_runs_give_identical_bits(gpu, D):
    """6. Exclusive ownership of the gX rows, the gq partials added in block order, no atomics."""
    X, lab, ids, w = _oracle(D, 64)[:4]
    a, b = _rows_run(gpu, X, ids, w)[3], _rows_run(gpu, X, ids, w)[3]
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())


def test_epanechnikov_state_answers_want_nearest_with_none(gpu, monkeypatch):
    """The stages set WANT_NEAREST and read LAST_NEAREST: after an Epanechnikov state it is None (nms_batch then
    selects for itself), whatever an earlier Gaussian call left there; without WANT_NEAREST it is left alone."""
    from parsenet_codebase_amd import mean_shift as MSM
    X = _inputs(64)[0].to(gpu)
    stale = torch.arange(3)
    monkeypatch.setattr(MSM, "LAST_NEAREST", stale)
    MSM.mean_shift_iterations_state(X, torch.tensor(BWS, device=gpu), 1, kernel_type="epa")
    assert MSM.LAST_NEAREST is stale
    monkeypatch.setattr(MSM, "WANT_NEAREST", True)
    MSM.mean_shift_iterations_state(X, torch.tensor(BWS, device=gpu), 1, kernel_type="epa")
    assert MSM.LAST_NEAREST is None


# ---------------------------------------------------------------------------------------------------------------
# 5. stages
# ---------------------------------------------------------------------------------------------------------------
SB, SN, SC = 2, 512, 4
# K = int(QUANTILE * 10000) = 16: the batched selection serves N / 16 >= 2 K; the 16th neighbour of a point lies
# inside its cluster of 128
QUANTILE = 0.0016


def _toy_batch(gpu, W):
    """SB shapes of two planes and two spheres, 128 points each, and a W-wide embedding of four well separated
    clusters that follows the segments."""
    from parsenet_codebase_amd import synthetic as S
    pts, nrm, lab, prim = [], [], [], []
    for b in range(SB):
        rng = np.random.RandomState(40 + b)
        parts = [S._plane(rng, 128), S._plane(rng, 128), S._sphere(rng, 128), S._sphere(rng, 128)]
        order = rng.permutation(SN)
        p, n = S.normalize_points(np.concatenate([q[0] for q in parts])[order],
                                  np.concatenate([q[1] for q in parts])[order], rng)
        pts.append(p); nrm.append(n)
        lab.append(np.repeat(np.arange(SC), 128)[order].astype(np.int64))
        prim.append(np.repeat([S.PRIM_PLANE, S.PRIM_PLANE, S.PRIM_SPHERE, S.PRIM_SPHERE], 128)[order].astype(np.int64))
    g = torch.Generator().manual_seed(17)
    code = torch.nn.functional.normalize(torch.randn(SC, W, generator=g), dim=1)
    emb = torch.stack([torch.nn.functional.normalize(
        code[torch.from_numpy(lab[b])] + 0.2 * torch.randn(SN, W, generator=g) / np.sqrt(W), dim=1) for b in range(SB)])
    logp = torch.log_softmax(torch.randn(SB, 10, SN, generator=g), 1)
    return (torch.from_numpy(np.stack(pts)).to(gpu), torch.from_numpy(np.stack(nrm)).to(gpu), np.stack(lab),
            np.stack(prim), emb.to(gpu), logp.to(gpu))


@pytest.mark.parametrize("W", [64, 50])
def test_cluster_shapes_with_the_epanechnikov_kernel(gpu, W):
    """fitting_eval.cluster_shapes(kernel_type="epa") at width 64 and at 50 (zero-padded to 64): every shape on
    the batched branch, one fused Epanechnikov call for the batch, and the cluster ids of the per-shape
    ``ev.ms.mean_shift(kernel_type="epa")`` — which are the four generating clusters."""
    from parsenet_codebase_amd import fitting_eval as FE, mean_shift as MSM
    from tests.test_fitting_batch_gpu import _evaluation
    torch.cuda.set_device(gpu)
    lab, emb = _toy_batch(gpu, W)[2], _toy_batch(gpu, W)[4]
    ev = _evaluation(gpu)
    before, epa = dict(FE.CALLS_CLUSTER), MSM.CALLS_EPA
    np.random.seed(3)
    pos = np.random.get_state()[2]
    clusters, calls = FE.cluster_shapes(ev, emb, QUANTILE, 10, kernel_type="epa")
    assert np.random.get_state()[2] == pos
    assert FE.CALLS_CLUSTER == {"batched": before["batched"] + SB, "per_shape": before["per_shape"]}
    assert MSM.CALLS_EPA == epa + 1 and calls == [1] * SB
    for b in range(SB):
        cen, bw, ids = clusters[b]
        assert cen.shape == (SC, W)
        with torch.no_grad():
            _, cen_r, bw_r, ids_r = ev.ms.mean_shift(emb[b], 10000, QUANTILE, 10, kernel_type="epa")
        assert abs(float(bw) - float(bw_r)) < 1e-5 * float(bw_r)
        assert np.array_equal(_canonical(ids), _canonical(ids_r.cpu().numpy()))
        assert np.array_equal(_canonical(ids), _canonical(lab[b]))
    assert MSM.CALLS_EPA == epa + 1 + SB


def test_training_fitting_loss_with_the_epanechnikov_kernel(gpu):
    """Evaluation.fitting_loss(kernel_type="epa") in training mode, shape by shape, through the batched stage
    (Epanechnikov state + centre rows) and through the per-shape path (``batched = False``: the dense backward over
    all rows): every shape on the batched branch, finite losses, and loss / means / IoUs / d loss / d embedding
    within the bars tests/test_fitting_width_gpu.py holds the batched stage to against the per-shape path.  Of its
    two sets the TIGHT one applies (loss and means 2e-4 / 2e-4 / 2e-5, IoUs 1e-9, gradient 5e-4 of its scale,
    cos > 0.99999): the loose set is for arms whose clusterings differ by the locality order of a planned launch, and
    here neither arm has one — N = 512 is below the plans' size and the Epanechnikov launches are dense anyway, so
    both arms take their bandwidth from the same selection kernel and their iterates from the same forward
    launches, and part only in the backward (rows in fp32 against the dense bf16 x 3 passes) and in the membership
    kernels."""
    import parsenet_codebase_amd.fitting_batch as FB
    from parsenet_codebase_amd import mean_shift as MSM
    from tests.test_fitting_batch_gpu import _evaluation
    torch.cuda.set_device(gpu)
    P, Nn, lab, prim, emb, logp = _toy_batch(gpu, 64)
    ev = _evaluation(gpu)
    outs = {}
    for mode in ("sequential", "batched"):
        ev.batched = mode == "batched"
        e = emb.clone().requires_grad_(True)
        np.random.seed(5)
        stage0, epa0 = dict(FB.CALLS_STAGE), MSM.CALLS_EPA
        res = [ev.fitting_loss(e[b:b + 1], P[b:b + 1], Nn[b:b + 1], lab[b:b + 1], prim[b:b + 1], logp[b:b + 1],
                               quantile=QUANTILE, iterations=10, lamb=0.1, kernel_type="epa") for b in range(SB)]
        sum(r[0][0].sum() for r in res).backward()
        outs[mode] = (res, e.grad.clone(), np.random.get_state()[2])
        assert MSM.CALLS_EPA == epa0 + SB
        if ev.batched:
            assert {k: FB.CALLS_STAGE[k] - stage0[k] for k in stage0} == {"batched": SB, "per_shape": 0}
    (rs, gs, ps), (rb, gb, pb) = outs["sequential"], outs["batched"]
    assert ps == pb
    tol = {0: 2e-4, 1: 2e-4, 2: 2e-5, 3: 1e-9, 4: 1e-9}
    for b in range(SB):
        ls, lb = rs[b][0], rb[b][0]
        ls, lb = [ls[0].detach()] + list(ls[1:]), [lb[0].detach()] + list(lb[1:])
        print("epa stage, shape %d: loss %.6g / %.6g, means %s / %s" % (b, float(ls[0]), float(lb[0]), ls[1:3], lb[1:3]))
        assert bool(torch.isfinite(lb[0]).all()) and bool(torch.isfinite(ls[0]).all())
        assert np.array_equal(_canonical(rs[b][1][1]), _canonical(rb[b][1][1]))
        assert np.array_equal(_canonical(rb[b][1][1]), _canonical(lab[b]))
        assert abs(float(ls[0]) - float(lb[0])) < tol[0] * abs(float(ls[0])) + 1e-9
        for k in (1, 2, 3, 4):
            assert (ls[k] is None) == (lb[k] is None)
            if ls[k] is not None:
                assert abs(ls[k] - lb[k]) < tol[k] * abs(ls[k]) + 1e-9, (b, k, ls[k], lb[k])
    assert bool(torch.isfinite(gb).all()) and float(gb.abs().max()) > 0
    scale = float(gs.abs().max())
    cos = float((gs.double().flatten() @ gb.double().flatten()) / (gs.double().norm() * gb.double().norm()))
    print("epa stage: gradient max |diff| %.2e of its scale, 1 - cos %.1e" % (float((gs - gb).abs().max()) / scale, 1 - cos))
    assert float((gs - gb).abs().max()) < 5e-4 * scale
    assert cos > 0.99999, cos
