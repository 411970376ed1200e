"""GPU: mean-shift at embedding widths other than 128 on the fused path (csrc/meanshift_w.hip: kernels at
widths 32 and 64; narrower rows zero-padded up to them, 65 ... 127 zero-padded to the 128-wide path).

Bars: the project's own for the 128-wide iterations (tests/test_parity_fullsize_bwd_gpu.py): iterates within
1e-5 absolute (unit rows), gradient within 5e-5 of its largest entry, cosine above 1 - 1e-8; the reference's
fixture at the bars tests/test_golden_gpu.py holds it to.  Every test names what it caught before the kernels
existed: then every width but 128 ran tensor-library expressions that keep the N x N kernel matrix of every
iteration for autograd, and nothing counted which path a call took."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
QUANTILE = 0.025


def _clustered_rows(n_clusters, N, D, noise, seed):
    """Unit rows around ``n_clusters`` random unit prototypes: noise of norm ~``noise`` whatever the width."""
    g = torch.Generator().manual_seed(seed)
    proto = torch.nn.functional.normalize(torch.randn(n_clusters, D, generator=g), dim=1)
    lab = torch.arange(N) % n_clusters
    emb = proto[lab] + noise * torch.randn(N, D, generator=g) / np.sqrt(D)
    return torch.nn.functional.normalize(emb, dim=1), lab.numpy()


def _oracle_bandwidth(X):
    """The oracle's own compute_bandwidth at the configs' quantile (all rows: independent of the shuffle)."""
    from oracle import ref_torch as R
    np.random.seed(3)
    with torch.no_grad():
        return float(torch.clamp(R.MeanShift().compute_bandwidth(X, X.shape[0], QUANTILE), min=0.003))


def _oracle_run(X, G_, bw, iterations=10):
    from oracle import ref_torch as R
    xr = X.clone().requires_grad_(True)
    out, _ = R.MeanShift().mean_shift_(xr, bw, iterations)
    (out * G_).sum().backward()
    return out.detach(), xr.grad.detach()


def _check(out_g, grad_g, out_r, grad_r, what):
    err = float((out_g.detach().cpu() - out_r).abs().max())
    gr, gg = grad_r.double(), grad_g.detach().cpu().double()
    gerr = float((gg - gr).abs().max()) / float(gr.abs().max())
    cos = float((gg.flatten() @ gr.flatten()) / (gg.norm() * gr.norm()))
    print("%s: iterates max |diff| %.2e, gradient %.2e of its largest entry, 1 - cos %.1e" % (what, err, gerr, 1 - cos))
    assert err < 1e-5, (what, err)
    assert gerr < 5e-5 and cos > 1 - 1e-8, (what, gerr, cos)


def _host_memory_gb():
    try:
        with open("/proc/meminfo") as fh:
            for line in fh:
                if line.startswith("MemAvailable:"):
                    return int(line.split()[1]) / 2 ** 20
    except OSError:
        pass
    return 0.0


def _partition_agreement(a, b):
    """Share of points on which two labelings agree after the best one-to-one renaming."""
    from scipy.optimize import linear_sum_assignment
    a, b = np.asarray(a).astype(np.int64), np.asarray(b).astype(np.int64)
    ua, ia = np.unique(a, return_inverse=True)
    ub, ib = np.unique(b, return_inverse=True)
    conf = np.bincount(ia * len(ub) + ib, minlength=len(ua) * len(ub)).reshape(len(ua), len(ub))
    r, c = linear_sum_assignment(-conf)
    return conf[r, c].sum() / float(a.size)


def test_reference_fixture_at_width_64_runs_on_the_width_kernels(gpu):
    """tests/golden/mean_shift_variants.npz (the REFERENCE's iterates and gradient: width 64, 300 points, 5
    iterations, gaussian kernel) at the bars of test_golden_gpu.py — and the call is counted by CALLS_W.
    Before: no such counter, and the call ran the N x N tensor expressions."""
    from parsenet_codebase_amd import mean_shift as MSM
    g = np.load(os.path.join(G, "mean_shift_variants.npz"), allow_pickle=False)
    X, w = torch.from_numpy(g["X"]).to(gpu), torch.from_numpy(g["w"]).to(gpu)
    assert X.shape == (300, 64)
    before, before128 = MSM.CALLS_W, dict(MSM.CALLS)
    xg = X.clone().requires_grad_(True)
    yg, _ = MSM.MeanShift().mean_shift_(xg, torch.tensor(float(g["b"]), device=gpu), 5, kernel_type="gaussian")
    (yg * w).sum().backward()
    assert MSM.CALLS_W == before + 1 and MSM.CALLS == before128

    def rel(a, b):
        a, b = a.detach().cpu().numpy().astype(np.float64), np.asarray(b, np.float64)
        return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))
    rf, rg = rel(yg, g["new_X_gaussian"]), rel(xg.grad, g["grad_gaussian"])
    print("reference fixture, width 64: iterates rel %.2e gradient rel %.2e" % (rf, rg))
    assert rf < 1e-5 and rg < 5e-5, (rf, rg)


@pytest.mark.parametrize("N", [300, 2049])
@pytest.mark.parametrize("D", [32, 64, 20, 50, 96])
def test_ten_iterations_and_their_gradient_against_the_oracle(gpu, D, N):
    """Ten iterations differentiated, against torch-CPU autograd through the oracle's N x N iterations, at the
    native widths 32 and 64 and the padded ones 20 (-> 32), 50 (-> 64: the public constructor's default
    embedding size) and 96 (-> 128); N is not a multiple of the 32-point tile.  Before: these widths ran
    the tensor expressions (this test then compared two N x N implementations); now it holds the kernels, their
    tail tiles and the padding to the bars of the 128-wide path."""
    from parsenet_codebase_amd import mean_shift as MSM
    X, _ = _clustered_rows(7, N, D, 0.3, 100 + D)
    G_ = torch.randn(N, D, generator=torch.Generator().manual_seed(N + D))
    bw = _oracle_bandwidth(X)
    out_r, grad_r = _oracle_run(X, G_, bw)
    w_before, c_before = MSM.CALLS_W, sum(MSM.CALLS.values())
    xg = X.to(gpu).requires_grad_(True)
    out_g, _ = MSM.MeanShift().mean_shift_(xg, torch.tensor(bw, device=gpu), 10)
    (out_g * G_.to(gpu)).sum().backward()
    if D <= 64:
        assert MSM.CALLS_W == w_before + 1 and sum(MSM.CALLS.values()) == c_before
    else:
        assert MSM.CALLS_W == w_before and sum(MSM.CALLS.values()) == c_before + 1
    assert out_g.shape == (N, D) and xg.grad.shape == (N, D)
    _check(out_g, xg.grad, out_r, grad_r, "width %d, N %d, bandwidth %.4f" % (D, N, bw))


@pytest.mark.parametrize("D", [32, 64])
def test_batch_of_two_with_two_bandwidths(gpu, D):
    """mean_shift_iterations on (B,N,D) with one bandwidth per item: each item against the oracle at ITS
    bandwidth.  Before: the (B,N,D) entry refused every width but 128 (the C ABI's argument check)."""
    from parsenet_codebase_amd import mean_shift as MSM
    N = 2049
    Xs = [_clustered_rows(5 + 4 * i, N, D, 0.4 + 0.2 * i, 40 + i)[0] for i in range(2)]
    G_ = torch.randn(2, N, D, generator=torch.Generator().manual_seed(8))
    bws = [_oracle_bandwidth(X) for X in Xs]
    assert abs(bws[0] - bws[1]) > 1e-3
    xg = torch.stack(Xs).to(gpu).requires_grad_(True)
    before = MSM.CALLS_W
    out_g = MSM.mean_shift_iterations(xg, torch.tensor(bws, device=gpu), 10)
    (out_g * G_.to(gpu)).sum().backward()
    assert MSM.CALLS_W == before + 1
    for i in range(2):
        out_r, grad_r = _oracle_run(Xs[i], G_[i], bws[i])
        _check(out_g[i], xg.grad[i], out_r, grad_r, "batch item %d, width %d, bandwidth %.4f" % (i, D, bws[i]))


def test_full_size_at_width_64_against_the_oracle(gpu):
    """Width 64 at the benchmark's size: N = 10 000, ten iterations, forward and gradient against the oracle's
    autograd (which keeps every N x N matrix: ~15 GB of host memory, slow).  Before: the product kept them too,
    on the GPU."""
    if _host_memory_gb() < 40:
        pytest.skip("the oracle's autograd keeps ~15 GB of N x N matrices; not enough host memory")
    from parsenet_codebase_amd import mean_shift as MSM
    torch.cuda.set_device(gpu)
    N, D = 10000, 64
    X, _ = _clustered_rows(9, N, D, 0.3, 4)
    G_ = torch.randn(N, D, generator=torch.Generator().manual_seed(11))
    bw = _oracle_bandwidth(X)
    out_r, grad_r = _oracle_run(X, G_, bw)
    before = MSM.CALLS_W
    xg = X.to(gpu).requires_grad_(True)
    out_g, _ = MSM.MeanShift().mean_shift_(xg, torch.tensor(bw, device=gpu), 10)
    (out_g * G_.to(gpu)).sum().backward()
    assert MSM.CALLS_W == before + 1
    _check(out_g, xg.grad, out_r, grad_r, "width 64, N 10 000, bandwidth %.4f" % bw)


def test_no_n_by_n_matrix_is_ever_allocated(gpu):
    """Width 64, N = 10 000, ten iterations forward + backward: the peak of the caching allocator rises by less
    than ONE N x N fp32 matrix (4 N^2 bytes) over the call — what "the N x N matrix never exists" promises,
    not a measurement.  Before: ten of them and their intermediates were kept for autograd (> 10 x the bound)."""
    from parsenet_codebase_amd import mean_shift as MSM
    torch.cuda.set_device(gpu)
    N, D = 10000, 64
    X, _ = _clustered_rows(9, N, D, 0.3, 4)
    xg = X.to(gpu).requires_grad_(True)
    G_ = torch.randn(N, D, generator=torch.Generator().manual_seed(11)).to(gpu)
    bw = torch.tensor(0.2, device=gpu)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out_g, _ = MSM.MeanShift().mean_shift_(xg, bw, 10)
    (out_g * G_).sum().backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print("width 64, N 10 000, 10 iterations fwd + bwd: peak rise %.1f MB (one N x N fp32 matrix: %.0f MB)"
          % (rise / 1e6, 4 * N * N / 1e6))
    assert rise < 4 * N * N, rise
    assert bool(torch.isfinite(xg.grad).all())


@pytest.mark.parametrize("D,W", [(50, 64), (96, 128), (20, 32)])
def test_padding_is_exact(gpu, D, W):
    """A D-wide input gives, bit for bit, the iterates and the gradient of the explicitly zero-padded W-wide
    input, sliced: zero columns are exact in every product and stay zero through the renormalisation.  Before:
    widths 50 and 64 were two different tensor-library GEMM shapes."""
    from parsenet_codebase_amd import mean_shift as MSM
    N = 2049
    X, _ = _clustered_rows(7, N, D, 0.3, 21)
    G_ = torch.randn(N, D, generator=torch.Generator().manual_seed(5)).to(gpu)
    bw = torch.tensor(_oracle_bandwidth(X), device=gpu)
    xa = X.to(gpu).requires_grad_(True)
    ya, _ = MSM.MeanShift().mean_shift_(xa, bw, 10)
    (ya * G_).sum().backward()
    xb = torch.nn.functional.pad(X, (0, W - D)).to(gpu).requires_grad_(True)
    yb, _ = MSM.MeanShift().mean_shift_(xb, bw, 10)
    (yb[:, :D] * G_).sum().backward()
    assert yb.shape == (N, W) and bool((yb[:, D:] == 0).all())
    assert torch.equal(ya.detach(), yb.detach()[:, :D])
    assert torch.equal(xa.grad, xb.grad[:, :D])


@pytest.mark.parametrize("D", [32, 64])
def test_two_runs_give_identical_bits(gpu, D):
    """Forward + backward twice on the same input, B = 2: identical bits (partial sums combined in a fixed
    order, no floating-point atomics), as every other workload of the project."""
    from parsenet_codebase_amd import mean_shift as MSM
    N = 2049
    X = torch.stack([_clustered_rows(6, N, D, 0.5, 60 + i)[0] for i in range(2)]).to(gpu)
    G_ = torch.randn(2, N, D, generator=torch.Generator().manual_seed(2)).to(gpu)
    bw = torch.tensor([0.15, 0.22], device=gpu)
    runs = []
    for _ in range(2):
        xg = X.clone().requires_grad_(True)
        out = MSM.mean_shift_iterations(xg, bw, 10)
        (out * G_).sum().backward()
        runs.append((out.detach().clone(), xg.grad.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert bool(torch.isfinite(runs[0][1]).all())


def test_whole_clustering_call_at_width_64(gpu):
    """MeanShift().mean_shift(X, N, 0.025, 10) at width 64 — bandwidth (the selection engine at C = 64), ten
    iterations on the width kernels, non-maximum suppression — on twelve well-separated clusters of 4 000 points:
    the labels equal the oracle's as a partition.  The input is one on which the oracle alone is stable (its
    fp32 and fp64 runs give the same partition).  Before: the iterations of this call ran the N x N path."""
    from oracle import ref_torch as R
    from parsenet_codebase_amd import mean_shift as MSM
    N, D = 4000, 64
    X, lab = _clustered_rows(12, N, D, 0.25, 7)
    np.random.seed(1)
    with torch.no_grad():
        _, cen_r, bw_r, lab_r = R.MeanShift().mean_shift(X, N, QUANTILE, 10)
    np.random.seed(1)
    with torch.no_grad():
        _, _, _, lab_r64 = R.MeanShift().mean_shift(X.double(), N, QUANTILE, 10)
    assert _partition_agreement(lab_r.numpy(), lab_r64.numpy()) == 1.0     # the oracle alone is stable here
    assert _partition_agreement(lab_r.numpy(), lab) == 1.0 and cen_r.shape[0] == 12
    before = MSM.CALLS_W
    np.random.seed(1)
    with torch.no_grad():
        new_X, cen_g, bw_g, lab_g = MSM.MeanShift().mean_shift(X.to(gpu), N, QUANTILE, 10)
    assert MSM.CALLS_W == before + 1
    # (dot products carry ~1e-7 on either side: 2e-7 of a squared K-th distance of ~b^2 = 0.1, i.e. ~1e-6 of
    # its root per row; the bar leaves the mean over the rows a factor of 100)
    assert abs(float(bw_g) - float(bw_r)) <= 1e-4 * float(bw_r)
    assert cen_g.shape[0] == cen_r.shape[0]
    assert _partition_agreement(lab_g.cpu().numpy(), lab_r.numpy()) == 1.0


def test_workspace_rebuilds_its_images_for_another_x(gpu):
    """The tile images of the data live in the workspace and are reused only for the very tensor they were
    built from, unmodified: another x, or the same one written to in place, gives what a fresh workspace gives
    (bit for bit), forward and backward; a non-fp32 bsq or a mis-shaped rsum is refused."""
    from parsenet_codebase_amd import kernels as K
    B, N, D = 1, 1000, 64
    xs = [_clustered_rows(5, N, D, 0.3, 70 + i)[0].unsqueeze(0).to(gpu).contiguous() for i in range(2)]
    gy = torch.randn(B, N, D, generator=torch.Generator().manual_seed(3)).to(gpu)
    bsq = torch.tensor([0.09], device=gpu)

    def fresh(x):
        y, r, n = K.meanshift_w_iter_fwd(x, x, bsq, K.MeanShiftWWorkspace(B, N, D, gpu))
        gx = torch.zeros_like(x)
        gq = K.meanshift_w_iter_bwd(gy, y, x, x, r, n, bsq, K.MeanShiftWWorkspace(B, N, D, gpu, backward=True), gx)
        return y, r, n, gq, gx
    want = [fresh(x) for x in xs]
    wf, wb = K.MeanShiftWWorkspace(B, N, D, gpu), K.MeanShiftWWorkspace(B, N, D, gpu, backward=True)
    for i in (0, 1, 0):
        y, r, n = K.meanshift_w_iter_fwd(xs[i], xs[i], bsq, wf)
        assert wf.holds_image_of(xs[i]) and not wf.holds_image_of(xs[1 - i])
        gx = torch.zeros_like(xs[i])
        gq = K.meanshift_w_iter_bwd(gy, y, xs[i], xs[i], r, n, bsq, wb, gx)
        for got, ref in zip((y, r, n, gq, gx), want[i]):
            assert torch.equal(got, ref)
    x = xs[0].clone()
    K.meanshift_w_iter_fwd(x, x, bsq, wf)
    x.copy_(xs[1])                                   # same tensor, new contents
    assert not wf.holds_image_of(x)
    y, r, n = K.meanshift_w_iter_fwd(x, x, bsq, wf)
    assert torch.equal(y, want[1][0]) and torch.equal(r, want[1][1])
    with pytest.raises(ValueError):
        K.meanshift_w_iter_fwd(x, x, bsq.double(), wf)
    with pytest.raises(ValueError):
        K.meanshift_w_iter_bwd(gy, y, x, x, r[:, :-1], n, bsq, wb, torch.zeros_like(x))
