"""GPU: the Epanechnikov kernel of MeanShift.mean_shift_ (src/mean_shift.py:64-68) on the fused, recompute-
backward kernels at embedding widths up to 128 — against the reference's own iterates and gradient, against
the torch-CPU oracle's autograd, and against the promise that nothing of size N x N is allocated.

The kernel's derivative jumps at the edge of its support, so a gradient is only well defined to the bars
below where the supports hold many points; every input here was first run through the oracle in fp32 and in
fp64 on the CPU and kept because the two differ by at most a quarter of the bar (figures with the cases)."""
import os

import numpy as np
import pytest
import torch

from tests.test_meanshift_gpu import _canonical, _clustered, _rel

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ITER_BAR, GRAD_BAR = 1e-5, 5e-5


def _oracle(X, b, w, iters):
    from oracle import ref_torch as R
    xr = X.clone().requires_grad_(True)
    yr, _ = R.MeanShift().mean_shift_(xr, b, iters, kernel_type="epa")
    (yr * w).sum().backward()
    return yr.detach(), xr.grad


def test_reference_fixture_runs_fused(gpu):
    """tests/golden/mean_shift_variants.npz (the reference's iterates and gradient, width 64, five iterations)
    at the bars of test_golden_gpu.py — and the call is one of the fused path's, not a tensor expression."""
    from parsenet_codebase_amd import mean_shift as MSM
    g = np.load(os.path.join(G, "mean_shift_variants.npz"), allow_pickle=False)
    X, w = torch.from_numpy(g["X"]).to(gpu), torch.from_numpy(g["w"]).to(gpu)
    before = MSM.CALLS_EPA
    xg = X.clone().requires_grad_(True)
    yg, same = MSM.MeanShift().mean_shift_(xg, torch.tensor(float(g["b"]), device=gpu), 5, kernel_type="epa")
    (yg * w).sum().backward()
    ei, eg = _rel(yg, torch.from_numpy(g["new_X_epa"])), _rel(xg.grad, torch.from_numpy(g["grad_epa"]))
    print("reference fixture, epa: iterates %.2e gradient %.2e" % (ei, eg))
    assert same is xg
    assert MSM.CALLS_EPA == before + 1
    assert ei < ITER_BAR and eg < GRAD_BAR


# (N, clusters, width, bandwidth): native 32 / 64 / 128, padded 20 / 50 / 96, N below and above a tile
# multiple, one and several column slices.  Supports of 38 ... 881 points per row; the oracle's own fp32 vs
# fp64 deviation is at most 4.8e-7 (iterates) and 8.9e-6 (gradient) over these rows.
CASES = [(2049, 6, 64, 0.30), (2049, 6, 64, 0.35), (2049, 6, 128, 0.30), (2049, 6, 32, 0.40), (300, 3, 64, 0.40),
         (300, 3, 50, 0.35), (4100, 5, 128, 0.30), (6000, 9, 64, 0.32), (2049, 6, 96, 0.30), (2049, 6, 20, 0.40)]


@pytest.mark.parametrize("N,C,d,b", CASES)
def test_iterates_and_gradient_against_the_oracle(gpu, monkeypatch, N, C, d, b):
    from parsenet_codebase_amd import mean_shift as MSM
    nearest = torch.arange(3)                       # stands for an earlier Gaussian call's answer
    monkeypatch.setattr(MSM, "LAST_NEAREST", nearest)
    X, _ = _clustered(N, C, 21 + d, spread=0.2, d=d)
    w = torch.randn(N, d, generator=torch.Generator().manual_seed(4))
    bt = torch.tensor(b)
    yr, gr = _oracle(X, bt, w, 10)
    before, others = MSM.CALLS_EPA, (dict(MSM.CALLS), MSM.CALLS_W, dict(MSM._AUTO))
    xg = X.to(gpu).requires_grad_(True)
    yg, _ = MSM.MeanShift().mean_shift_(xg, bt.to(gpu), 10, kernel_type="epa")
    (yg * w.to(gpu)).sum().backward()
    ei, eg = _rel(yg, yr), _rel(xg.grad, gr)
    print("epa N %d C %d d %d b %.2f: iterates %.2e gradient %.2e" % (N, C, d, b, ei, eg))
    assert MSM.CALLS_EPA == before + 1
    assert (dict(MSM.CALLS), MSM.CALLS_W, dict(MSM._AUTO)) == others      # dense, no plan, no probing
    assert MSM.LAST_NEAREST is nearest
    assert yg.shape == (N, d) and xg.grad.shape == (N, d)
    assert ei < ITER_BAR
    assert eg < GRAD_BAR


@pytest.mark.parametrize("d", [64, 128])
def test_batch_of_two_with_two_bandwidths(gpu, d):
    """(B,N,d) with one bandwidth per item: each item against its own oracle run.  (Oracle fp32 vs fp64 of the
    item added to the table above, width 128 at b = 0.35: 3.2e-7 / 9.7e-6.)"""
    from parsenet_codebase_amd import mean_shift as MSM
    N, bs = 2049, (0.30, 0.35)
    X, _ = _clustered(N, 6, 21 + d, spread=0.2, d=d)
    w = torch.randn(N, d, generator=torch.Generator().manual_seed(4))
    xg = torch.stack([X, X]).to(gpu).requires_grad_(True)
    yg = MSM.mean_shift_iterations(xg, torch.tensor(bs, device=gpu), 10, kernel_type="epa")
    (yg * w.to(gpu)).sum().backward()
    for i, b in enumerate(bs):
        yr, gr = _oracle(X, torch.tensor(b), w, 10)
        ei, eg = _rel(yg[i], yr), _rel(xg.grad[i], gr)
        print("epa batch item %d d %d b %.2f: iterates %.2e gradient %.2e" % (i, d, b, ei, eg))
        assert ei < ITER_BAR
        assert eg < GRAD_BAR


@pytest.mark.parametrize("d", [64, 128])
def test_no_n_by_n_matrix_is_ever_allocated(gpu, d):
    """N = 10 000, ten iterations forward + backward: the peak of the caching allocator rises by less than ONE
    N x N fp32 matrix (4 N^2 bytes) over the call — the promise, not a measurement.  The tensor expressions
    kept several such matrices per iteration for autograd (more than 10 x the bound)."""
    from parsenet_codebase_amd import mean_shift as MSM
    torch.cuda.set_device(gpu)
    N = 10000
    X, _ = _clustered(N, 9, 21 + d, spread=0.2, d=d)
    xg = X.to(gpu).requires_grad_(True)
    G_ = torch.randn(N, d, generator=torch.Generator().manual_seed(11)).to(gpu)
    bw = torch.tensor(0.3, device=gpu)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out_g, _ = MSM.MeanShift().mean_shift_(xg, bw, 10, kernel_type="epa")
    (out_g * G_).sum().backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print("epa width %d, N 10 000, 10 iterations fwd + bwd: peak rise %.1f MB (one N x N fp32 matrix: %.0f MB)"
          % (d, rise / 1e6, 4 * N * N / 1e6))
    assert rise < 4 * N * N, rise
    assert bool(torch.isfinite(out_g).all()) and bool(torch.isfinite(xg.grad).all())


@pytest.mark.parametrize("d,N", [(32, 2049), (64, 4100), (128, 4100)])
def test_two_runs_give_identical_bits(gpu, d, N):
    """Partial sums are combined in slice order, no atomics: iterates and gradient repeat bit for bit."""
    from parsenet_codebase_amd import mean_shift as MSM
    X, _ = _clustered(N, 6, 21 + d, spread=0.2, d=d)
    w = torch.randn(N, d, generator=torch.Generator().manual_seed(4)).to(gpu)
    runs = []
    for _ in range(2):
        xg = X.to(gpu).requires_grad_(True)
        yg, _ = MSM.MeanShift().mean_shift_(xg, torch.tensor(0.35, device=gpu), 10, kernel_type="epa")
        (yg * w).sum().backward()
        runs.append((yg.detach().clone(), xg.grad.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert bool(torch.isfinite(runs[0][1]).all())


@pytest.mark.parametrize("d", [64, 128])
def test_whole_clustering_call(gpu, d):
    """mean_shift(X, 10000, 0.015, 10, kernel_type="epa") on well separated clusters: bandwidth, and the labels
    as a partition (see test_full_mean_shift_partition).  (K = int(0.015 * 10000) = 150 stays inside a cluster
    of ~250 points; on the CPU the oracle's partition of these inputs is the generating one.)"""
    from oracle import ref_torch as R
    from parsenet_codebase_amd import mean_shift as MSM
    N = 1500
    X, lab = _clustered(N, 6, 21 + d, spread=0.2, d=d)
    np.random.seed(0)
    newr, cr, bwr, lr = R.MeanShift().mean_shift(X, 10000, 0.015, 10, kernel_type="epa")
    before = MSM.CALLS_EPA
    np.random.seed(0)
    newg, cg, bwg, lg = MSM.MeanShift().mean_shift(X.to(gpu), 10000, 0.015, 10, kernel_type="epa")
    assert MSM.CALLS_EPA == before + 1
    assert abs(bwg.item() - bwr.item()) / bwr.item() < 1e-5
    assert cg.shape == cr.shape
    assert np.array_equal(_canonical(lg.cpu().numpy()), _canonical(lr.numpy()))
    assert np.array_equal(_canonical(lr.numpy()), _canonical(lab.numpy()))


def test_other_arithmetics_keep_the_tensor_expressions(gpu, monkeypatch):
    """PARSENET_MS_ARITH = f32: the fused Epanechnikov kernel is bf16 x 3 only, so the call runs the tensor
    expressions as before — the arithmetic asked for is the arithmetic that runs — and matches the oracle."""
    from parsenet_codebase_amd import mean_shift as MSM
    monkeypatch.setattr(MSM, "ARITH", "f32")
    N, d, b = 2049, 64, 0.30
    X, _ = _clustered(N, 6, 21 + d, spread=0.2, d=d)
    w = torch.randn(N, d, generator=torch.Generator().manual_seed(4))
    yr, gr = _oracle(X, torch.tensor(b), w, 10)
    before = MSM.CALLS_EPA
    xg = X.to(gpu).requires_grad_(True)
    yg, _ = MSM.MeanShift().mean_shift_(xg, torch.tensor(b, device=gpu), 10, kernel_type="epa")
    (yg * w.to(gpu)).sum().backward()
    assert MSM.CALLS_EPA == before
    assert _rel(yg, yr) < ITER_BAR
    assert _rel(xg.grad, gr) < GRAD_BAR


def test_wrapper_refuses_a_plan_for_the_epanechnikov_kernel(gpu):
    """The library's refusal (tests/test_meanshift_epa_abi.py) reaches Python as an error, before any launch."""
    from parsenet_codebase_amd import kernels as K
    N = 4096
    x = torch.nn.functional.normalize(torch.randn(1, N, 128, generator=torch.Generator().manual_seed(1)), dim=2).to(gpu)
    bsq = torch.full((1,), 0.09, device=gpu)
    img, ws = K.meanshift_x3_split(x), K.MeanShiftWorkspace(1, N, 128, x.device)
    plan = torch.zeros(K.meanshift_x3_plan_bytes(1, N), dtype=torch.uint8, device=gpu)
    with pytest.raises(RuntimeError, match="plan"):
        K.meanshift_x3_iter_fwd(x, img, bsq, ws, plan, kind=K.KERNEL_EPANECHNIKOV)
    y, r, n = K.meanshift_x3_iter_fwd(x, img, bsq, ws, None, kind=K.KERNEL_EPANECHNIKOV)
    assert bool(torch.isfinite(y).all()) and float(r.min()) > 0.7      # (a point is in its own support: K = 3/4 there)
