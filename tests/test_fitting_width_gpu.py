"""GPU: the batched fitting stage, the evaluation-mode clustering and the embedding loss at embedding widths below
128 — the row-restricted mean-shift backward (csrc/meanshift_rows.hip) and the membership / triplet kernels
(csrc/fused.hip) at widths 32 and 64, widths in between zero-padded to them.

Every bar is the project's own for the 128-wide twin of the same check and is named where it is used.  Before
these instantiations existed the C entry points refused every width but 128, ``fitting_batch._fitting_stage`` sent
every shape of a narrower embedding alone through ``ev.guard_mean_shift`` (one host synchronisation per shape, an
autograd graph through all N rows) and nothing counted which path a call took."""
import numpy as np
import pytest
import torch

from tests.test_fitting_batch_gpu import _evaluation
from tests.test_meanshift_width_gpu import _check, _clustered_rows, _oracle_bandwidth, _oracle_run

pytestmark = pytest.mark.gpu


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


# ---------------------------------------------------------------------------------------------------------------
# 1. centre rows: row backward = dense backward = oracle
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [3000, 10000])
@pytest.mark.parametrize("D", [32, 64])
def test_row_backward_equals_dense_backward_and_the_oracle(gpu, D, N):
    """B = 2, ten iterations, the gradient entering at 40 centre rows (repeated ids among them):
    ``centre_rows`` on the forward-only state against ``mean_shift_iterations(...)[ids]`` back-propagated through
    the dense passes, and at N = 3 000 both against torch-CPU autograd through the oracle's N x N iterations.
    Bars of tests/test_meanshift_width_gpu.py: iterates 1e-5, gradient 5e-5 of its largest entry, 1 - cos < 1e-8.
    Before: ``pn_meanshift_rows_bwd_f32: D must be 128``."""
    from parsenet_codebase_amd import mean_shift as MSM
    torch.cuda.set_device(gpu)
    B, R = 2, 40
    Xs = [_clustered_rows(7 + 2 * i, N, D, 0.3, 300 + D + i)[0] for i in range(B)]
    bws = [_oracle_bandwidth(X) for X in Xs]
    g = torch.Generator().manual_seed(N + D)
    ids = torch.randint(0, N, (B, R), generator=g)
    ids[:, 5] = ids[:, 4]                           # a repeat with gradient in both entries ...
    ids[:, 30:] = ids[:, :1]                        # ... and a repeated tail, as the padded centre lists have
    w = torch.randn(B, R, D, generator=g)
    X = torch.stack(Xs).to(gpu)
    bw = torch.tensor(bws, device=gpu)
    idg, wg = ids.to(gpu), w.to(gpu)
    before = MSM.CALLS_W
    xd = X.clone().requires_grad_(True)
    yd = MSM.mean_shift_iterations(xd, bw, 10)
    (torch.gather(yd, 1, idg.unsqueeze(2).expand(-1, -1, D)) * wg).sum().backward()
    xr = X.clone().requires_grad_(True)
    new_X, state = MSM.mean_shift_iterations_state(xr, bw, 10)
    assert MSM.CALLS_W == before + 2 and not new_X.requires_grad and state.inv is None
    c = MSM.centre_rows(xr, state, idg)
    assert torch.equal(c, torch.gather(new_X, 1, idg.unsqueeze(2).expand(-1, -1, D)))
    (c * wg).sum().backward()
    assert bool(torch.isfinite(xr.grad).all())
    for b in range(B):
        _check(new_X[b], xr.grad[b], yd[b].detach().cpu(), xd.grad[b].cpu(),
               "rows against dense, width %d, N %d, item %d" % (D, N, b))
    if N > 3000:
        return
    for b in range(B):
        G_ = torch.zeros(N, D).index_add_(0, ids[b], w[b])
        out_r, grad_r = _oracle_run(Xs[b], G_, bws[b])
        _check(new_X[b], xr.grad[b], out_r, grad_r, "rows against the oracle, width %d, item %d" % (D, b))
        _check(yd[b], xd.grad[b], out_r, grad_r, "dense against the oracle, width %d, item %d" % (D, b))


def test_selection_engine_serves_the_narrow_widths(gpu):
    """The stage's bandwidth (dot_kth_x3, then dot_select's value form) and NMS (dot_select, k = 1) at C = 32 and
    64 on the benchmark's size: they take their kernel route (None would send the stage to the per-shape path)
    and agree with a tensor-library topk / first arg-max on the same rows."""
    from parsenet_codebase_amd import kernels as K
    from parsenet_codebase_amd.mean_shift import _first_argmax
    for C in (32, 64):
        x = _clustered_rows(9, 10000, C, 0.3, C)[0].unsqueeze(0).to(gpu)
        y = _clustered_rows(9, 10000, C, 0.3, C + 1)[0].unsqueeze(0).to(gpu)
        a, b = K.dot_kth_x3(x, x, 250), K.dot_select(x, x, 250, want_value=True)
        c = K.dot_select(x, y, 1, want_value=False)
        assert a is not None and b is not None and c is not None, C
        ref = torch.topk(x[0] @ x[0].t(), 250, dim=1)[0][:, -1]
        clear = (a[1][0] == 0) & (b[1][0] == 0)
        assert float((a[0][0] - ref).abs()[clear].max()) < 1e-6 and float((b[0][0] - ref).abs()[clear].max()) < 1e-6
        d = x[0] @ y[0].t()
        top2 = torch.topk(d, 2, dim=1)[0]
        sure = (c[1][0] == 0) & (top2[:, 0] - top2[:, 1] > 1e-5)      # (rows whose maximum no rounding can move)
        assert int(sure.sum()) > 9000
        assert torch.equal(c[0][0, :, 0][sure], _first_argmax(d, 1)[sure])


# ---------------------------------------------------------------------------------------------------------------
# 2. memberships
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncls", [[1, 5, 16], [33, 2, 49], [12, 12, 7], [20, 1, 32]])
@pytest.mark.parametrize("D", [32, 64])
def test_membership_kernels_against_fp64(gpu, D, ncls):
    """Wraw, weights_normalize and its gradients onto centres and embedding at widths 32 and 64, CP = 16, 32 and
    64 (one cluster and padded rows among them), against ``weights_normalize_batch`` evaluated in float64 on the
    same centres; labels against the first arg-max.  Bars of tests/test_fused_gpu.py::test_membership_kernels:
    Wraw 2e-6 relative, Wn 2e-5 absolute, gradients 2e-4 of their largest entry.
    Before: ``pn_membership_fwd_f32: D=64 CP=16 (D = 128 and CP in {16, 32, 64} supported)``."""
    from parsenet_codebase_amd import fitting_batch as FB, kernels as K
    from parsenet_codebase_amd.mean_shift import _first_argmax
    torch.manual_seed(2)
    B, N = len(ncls), 3000
    Cp = max(ncls)
    emb = torch.nn.functional.normalize(torch.randn(B, N, D, device=gpu), dim=2)
    pick = torch.randint(0, N, (B, Cp), device=gpu)
    cen = torch.gather(emb, 1, pick.unsqueeze(2).expand(-1, -1, D)) + 0.05 * torch.randn(B, Cp, D, device=gpu)
    ncl = torch.tensor(ncls, device=gpu)
    cen = cen * (torch.arange(Cp, device=gpu).unsqueeze(0) < ncl.unsqueeze(1)).unsqueeze(2)    # padded rows: zeros
    bw = torch.tensor([0.3, 0.11, 0.45][:B], device=gpu)
    g = torch.randn(B, Cp, N, device=gpu)
    before = dict(FB.CALLS_MEMBERSHIP)
    c1, e1 = cen.clone().requires_grad_(True), emb.clone().requires_grad_(True)
    Wn1, Wraw1 = FB.memberships(c1, e1, bw, ncl)
    (Wn1[:, :Cp] * g).sum().backward()
    assert FB.CALLS_MEMBERSHIP["fused"] == before["fused"] + 1 and FB.CALLS_MEMBERSHIP["tensor"] == before["tensor"]
    c2, e2 = cen.double().requires_grad_(True), emb.double().requires_grad_(True)
    Wraw2 = torch.bmm(c2, e2.transpose(1, 2))
    Wn2 = FB.weights_normalize_batch(Wraw2, bw.double(), ncl)
    (Wn2 * g.double()).sum().backward()
    CP = Wn1.shape[1]
    assert CP == (16 if Cp <= 16 else 32 if Cp <= 32 else 64)
    if CP > Cp:
        assert float(Wn1[:, Cp:].abs().max()) == 0
    figures = (_rel(Wraw1[:, :Cp], Wraw2), float((Wn1[:, :Cp].double() - Wn2).abs().max()), _rel(c1.grad, c2.grad),
               _rel(e1.grad, e2.grad))
    print("memberships, width %d, ncl %s: Wraw rel %.2e, Wn abs %.2e, d centres rel %.2e, d embedding rel %.2e"
          % ((D, ncls) + figures))
    assert figures[0] < 2e-6
    assert figures[1] < 2e-5
    assert figures[2] < 2e-4 and figures[3] < 2e-4
    cpad = torch.nn.functional.pad(cen, (0, 0, 0, CP - Cp))
    Wraw, _, _, _, lab = K.membership_fwd(cpad, emb, bw, ncl, 1e-7, want_labels=True)
    valid = torch.arange(CP, device=gpu).view(1, CP, 1) < ncl.view(B, 1, 1)
    sc = torch.where(valid, Wraw, torch.full_like(Wraw, float("-inf")))
    assert torch.equal(lab, _first_argmax(sc, 1))


# ---------------------------------------------------------------------------------------------------------------
# 3. triplet loss
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num", [30, 7])
@pytest.mark.parametrize("D", [32, 50, 64])
def test_triplet_loss_fused_at_narrow_widths(gpu, D, num, monkeypatch):
    """EmbeddingLoss.triplet_loss at widths 32, 50 (zero-padded to 64) and 64: the fused kernels against the
    tensor-expression branch (``losses.FUSED = False``), same numpy seed, same consumption of numpy's generator.
    Bars of tests/test_fused_gpu.py::test_triplet_loss_kernel: loss 2e-6, gradient 2e-5, both relative.
    Before: no ``CALLS_TRIPLET_FUSED``, and these widths ran the tensor expressions in both arms."""
    from parsenet_codebase_amd import losses
    B, N, S = 3, 400, 6
    rng = np.random.RandomState(0)
    labels = rng.randint(0, S, (B, N))
    if num < 30:
        N = 40
        labels = labels[:, :N] % 8          # N // S + 1 < 30 -> fewer samples per segment
    out = torch.randn(B, D, N, device=gpu)
    res = {}
    for fused in (True, False):
        monkeypatch.setattr(losses, "FUSED", fused)
        before = losses.CALLS_TRIPLET_FUSED
        o = out.clone().requires_grad_(True)
        np.random.seed(5)
        l = losses.EmbeddingLoss(margin=1.0).triplet_loss(o, labels)
        l.sum().backward()
        assert (losses.CALLS_TRIPLET_FUSED > before) == fused
        res[fused] = (l.detach().clone(), o.grad.clone(), np.random.get_state()[2], np.random.get_state()[1][:4].tolist())
    assert res[True][2] == res[False][2] and res[True][3] == res[False][3]
    assert res[True][1].shape == (B, D, N)
    figures = (_rel(res[True][0], res[False][0]), _rel(res[True][1], res[False][1]))
    print("triplet, width %d, num %d: loss rel %.2e, gradient rel %.2e" % ((D, num) + figures))
    assert figures[0] < 2e-6
    assert figures[1] < 2e-5


# ---------------------------------------------------------------------------------------------------------------
# 4. the stage
# ---------------------------------------------------------------------------------------------------------------
# Shape triples tried for the own-clustering arm (every shape must come out of the per-shape path with at most 49
# clusters, and of the batched stage without a tie flag): the first one, the 128-wide test's, is the one in use.
SEEDS = (3, 8, 21)


def _structured_batch_w(gpu, B, N, seeds, W, noise):
    """tests/test_fitting_batch_gpu.py::_structured_batch at width W: ``code = randn(32, W)``, and the noise scaled
    per component as ``_clustered_rows`` does — noise * sqrt(128 / W) — so that its norm, and with it the
    crispness of the clusters, is the 128-wide batch's."""
    from parsenet_codebase_amd import synthetic
    pts, nrm, lab, prim = [], [], [], []
    for s in seeds:
        p, n, l, t = synthetic.make_shape(s, N)
        pts.append(p); nrm.append(n); lab.append(l); prim.append(t)
    g = torch.Generator().manual_seed(99)
    code = torch.nn.functional.normalize(torch.randn(32, W, generator=g), dim=1)
    per = noise * float(np.sqrt(128.0 / W))
    emb = torch.stack([torch.nn.functional.normalize(
        code[torch.from_numpy(lab[b]).long()] + per * torch.randn(N, W, generator=g), dim=1) for b in range(B)])
    logp = torch.log_softmax(torch.randn(B, 10, N, generator=g), 1)
    return (torch.from_numpy(np.stack(pts)).to(gpu), torch.from_numpy(np.stack(nrm)).to(gpu), np.stack(lab),
            np.stack(prim), emb.to(gpu), logp.to(gpu))


@pytest.mark.parametrize("N,shared_clustering", [(3000, True), (10000, True), (10000, False)])
@pytest.mark.parametrize("W", [64, 50])
def test_batched_stage_equals_shape_by_shape_at_narrow_widths(gpu, W, N, shared_clustering, monkeypatch):
    """tests/test_fitting_batch_gpu.py::test_batched_stage_equals_shape_by_shape at widths 64 and 50, same bars.
    Shared clustering (``bandwidth_batch`` -> None: both arms cluster shape by shape): ids equal, 2e-4 / 2e-5 /
    1e-9, gradient 5e-4 of its scale, cos > 0.99999, and ``memberships()`` ran the fused kernels.  Own clustering:
    equal partitions, the loose bars, cos > 0.9 — and every shape took the batched path (``CALLS_STAGE``).
    Before: ``per_shape`` would have advanced by B (and did not exist)."""
    import parsenet_codebase_amd.fitting_batch as FB
    torch.cuda.set_device(gpu)
    B = 3
    noise = 0.01 if N == 3000 else (0.04 if shared_clustering else 0.035)      # (the 128-wide test's)
    P, Nn, lab, prim, emb, logp = _structured_batch_w(gpu, B, N, SEEDS, W, noise)
    ev = _evaluation(gpu)
    if shared_clustering:
        monkeypatch.setattr(FB, "bandwidth_batch", lambda *a, **k: None)
    outs = {}
    for mode in ("sequential", "batched"):           # (sequential first: it shows what the per-shape path finds)
        ev.batched = mode == "batched"
        e = emb.clone().requires_grad_(True)
        np.random.seed(5)
        stage0, member0 = dict(FB.CALLS_STAGE), dict(FB.CALLS_MEMBERSHIP)
        if ev.batched:
            res = ev.fitting_losses(e, P, Nn, lab, prim, logp, quantile=0.025, iterations=10, lamb=0.1)
        else:
            res = [ev.fitting_loss(e[b:b + 1], P[b:b + 1], Nn[b:b + 1], lab[b:b + 1], prim[b:b + 1], logp[b:b + 1],
                                   quantile=0.025, iterations=10, lamb=0.1) for b in range(B)]
        sum(r[0][0].sum() for r in res).backward()
        outs[mode] = (res, e.grad.clone(), np.random.get_state()[2], np.random.get_state()[1][:4].tolist())
        if not ev.batched:
            nclusters = [int(np.unique(r[1][1]).size) for r in res]
            print("width %d, N %d, seeds %s: clusters per shape on the per-shape path %s" % (W, N, SEEDS, nclusters))
            assert max(nclusters) <= 49, nclusters
            continue
        took = {k: FB.CALLS_STAGE[k] - stage0[k] for k in stage0}
        if shared_clustering:
            assert took == {"batched": 0, "per_shape": B}
            assert FB.CALLS_MEMBERSHIP["fused"] == member0["fused"] + 1
            assert FB.CALLS_MEMBERSHIP["tensor"] == member0["tensor"]
        else:
            assert took == {"batched": B, "per_shape": 0}, took
    (rs, gs, ps, ks), (rb, gb, pb, kb) = outs["sequential"], outs["batched"]
    assert ps == pb and ks == kb                      # numpy's RNG stream advanced identically
    assert gb.shape == (B, N, W)
    tight = shared_clustering
    tol = {0: 2e-4 if tight else 0.25, 1: 2e-4 if tight else 2e-2, 2: 2e-5 if tight else 0.3, 3: 1e-9, 4: 1e-9}

    def canon(l):
        _, first = np.unique(l, return_index=True)
        remap = {int(v): i for i, v in enumerate(l[np.sort(first)])}
        return np.array([remap[int(v)] for v in l])
    for b in range(B):
        ls, lb = rs[b][0], rb[b][0]
        if tight:
            assert np.array_equal(rs[b][1][1], rb[b][1][1])                   # cluster ids
        else:
            assert np.array_equal(canon(rs[b][1][1]), canon(rb[b][1][1]))     # same partition
        print("width %d, N %d, shape %d: loss %.6g / %.6g, means %s / %s" % (W, N, b, float(ls[0]), float(lb[0]),
                                                                          ls[1:3], lb[1:3]))
        assert abs(float(ls[0]) - float(lb[0])) < tol[0] * abs(float(ls[0])) + 1e-9, (b, float(ls[0]), float(lb[0]))
        for k in (1, 2, 3, 4):
            assert (ls[k] is None) == (lb[k] is None)
            if ls[k] is not None:
                assert abs(ls[k] - lb[k]) < tol[k] * abs(ls[k]) + 1e-9, (b, k, ls[k], lb[k])
        if not tight:
            continue
        ks_, kb_ = rs[b][1][0], rb[b][1][0]
        assert sorted(ks_) == sorted(kb_)
        for key in ks_:
            assert (ks_[key] is None) == (kb_[key] is None)
            if ks_[key] is not None:
                assert ks_[key][0] == kb_[key][0]
        assert torch.allclose(rs[b][1][2], rb[b][1][2], atol=1e-6)
    scale = float(gs.abs().max())
    cos = float((gs.double().flatten() @ gb.double().flatten()) / (gs.double().norm() * gb.double().norm()))
    print("width %d, N %d, %s clustering: gradient max |diff| %.2e of its scale, 1 - cos %.1e"
          % (W, N, "shared" if tight else "own", float((gs - gb).abs().max()) / scale, 1 - cos))
    if tight:
        assert float((gs - gb).abs().max()) < 5e-4 * scale, float((gs - gb).abs().max()) / scale
        assert cos > 0.99999, cos
    else:
        assert cos > 0.9, cos


# ---------------------------------------------------------------------------------------------------------------
# 5. evaluation mode
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [64, 50])
def test_evaluation_clustering_takes_the_batched_branch(gpu, W):
    """fitting_eval.cluster_shapes at widths 64 and 50 (padded): every shape on the batched branch, the labels
    equal, as a partition, those of ``MeanShift.guard_mean_shift`` shape by shape; centres come back D wide and
    numpy's generator is left where it was.  Before: ``bandwidth_batch(...) if D == 128 else None``."""
    from parsenet_codebase_amd import fitting_eval as FE
    from parsenet_codebase_amd.mean_shift import MeanShift
    from tests.test_meanshift_width_gpu import _partition_agreement
    torch.cuda.set_device(gpu)
    B, N = 2, 10000
    emb = _structured_batch_w(gpu, B, N, SEEDS[:B], W, 0.01)[4]
    ev = _evaluation(gpu)
    before = dict(FE.CALLS_CLUSTER)
    np.random.seed(3)
    pos = np.random.get_state()[2]
    clusters, calls = FE.cluster_shapes(ev, emb, 0.025, 10)
    assert np.random.get_state()[2] == pos
    assert FE.CALLS_CLUSTER["batched"] == before["batched"] + B and FE.CALLS_CLUSTER["per_shape"] == before["per_shape"]
    assert calls == [1] * B
    for b in range(B):
        cen, bw, ids = clusters[b]
        assert cen.shape[1] == W and cen.shape[0] == np.unique(ids).size
        np.random.seed(4)
        with torch.no_grad():
            cen_r, bw_r, ids_r = MeanShift().guard_mean_shift(emb[b], 0.025, 10)
        assert cen.shape[0] == cen_r.shape[0]
        assert _partition_agreement(ids, ids_r.cpu().numpy()) == 1.0
