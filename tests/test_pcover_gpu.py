"""GPU: point coverage of the fitted primitives (metrics.p_coverage, csrc/cover.hip) against the fixture the reference
wrote (tests/golden/make_golden_pcover.py).  The bar of a primitive type is 4 x noise[type], the reference's own
fp32 error (fp32 against fp64 on the same inputs) stored in the fixture; a point's bar is that of the type that wins
it.  All shapes of the fixture live in the unit box, for which the bars were measured."""
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
NPARAM = {"plane": 2, "sphere": 2, "cylinder": 3, "cone": 3, "open-spline": 1, "closed-spline": 1}


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(ROOT, "tests", "golden", "pcover.npz"), allow_pickle=False)


def _bars(fx):
    return {str(t): 4.0 * float(n) for t, n in zip(fx["types"], fx["noise"])}


def _entry(fx, name, dev):
    return [name] + [torch.from_numpy(fx["%s_p%d" % (name, i)]).to(dev) for i in range(NPARAM[name])]


def _shape(fx, tag, dev, key=lambda i: i):
    """(points, parameter dict in the fixture's order, names of the entries that are not None)"""
    names = [str(x) for x in fx[tag + "_names"]]
    prm = {key(i): (None if n == "none" else _entry(fx, n, dev)) for i, n in enumerate(names)}
    return torch.from_numpy(fx[tag + "_points"]).to(dev), prm, [n for n in names if n != "none"]


def _run(monkeypatch, path, points, params, **kw):
    from parsenet_codebase_amd import metrics
    monkeypatch.setenv("PARSENET_PCOVER", path)
    return metrics.p_coverage_batch(points, params, **kw)


def test_fused_against_the_reference(gpu, fx, monkeypatch):
    """Shape a (1 237 points, seven primitives and a None entry): dmin within the bar of the winning type, cover and
    arg equal off the excused points, the lower of the two identical planes, the mean within the largest bar."""
    from parsenet_codebase_amd import metrics
    bars = _bars(fx)
    pts, prm, live = _shape(fx, "a", gpu, key=lambda i: 10 + 3 * i)      # keys 10, 13, ..: arg comes back as keys
    before = dict(metrics.CALLS_PCOVER)
    (mean, cover, dmin, key), = _run(monkeypatch, "fused", [pts], [prm], return_points=True)
    assert metrics.CALLS_PCOVER["fused"] == before["fused"] + 1 and metrics.CALLS_PCOVER["tensor"] == before["tensor"]
    assert mean.dim() == 0 and cover.dim() == 0 and dmin.dtype == torch.float32 and key.dtype == torch.int64
    dmin, key = dmin.cpu().numpy(), key.cpu().numpy()
    assert ((key - 10) % 3 == 0).all()
    row = (key - 10) // 3
    assert row.min() >= 0 and row.max() < len(live)                       # the None entry (key 31) never wins
    bar = np.asarray([bars[live[r]] for r in row])
    err = np.abs(dmin.astype(np.float64) - fx["a_min32"].astype(np.float64))
    print("dmin: max |fused - reference fp32| / bar = %.3f (max error %.3e)" % ((err / bar).max(), err.max()))
    assert (err <= bar).all()
    near = fx["a_near_cover"]
    assert near.mean() <= 0.01
    assert np.array_equal((dmin < 0.01)[~near], (fx["a_min32"] < 0.01)[~near])
    tie = fx["a_near_tie"]
    assert tie.mean() <= 0.02
    want = fx["a_d64"].argmin(0)                                          # the first of equal rows
    print("arg: %d of %d points differ off the %d excused ones" % ((row != want)[~tie].sum(), row.size, tie.sum()))
    assert np.array_equal(row[~tie], want[~tie])
    planes = [i for i, n in enumerate(live) if n == "plane"]
    assert len(planes) == 2 and (row == planes[0]).any() and not (row == planes[1]).any()
    assert all((row == r).any() for r in range(len(live)) if r != planes[1])
    print("mean %.9f (reference %.9f), cover %.6f (reference %.6f)"
          % (mean.item(), float(fx["a_mean32"]), cover.item(), float(fx["a_cover32"])))
    assert abs(mean.item() - float(fx["a_mean32"])) <= max(bars.values())
    assert abs(cover.item() - float(fx["a_cover32"])) <= near.mean() + 1e-6
    m1, c1 = metrics.p_coverage(fx["a_points"], prm)                      # numpy points, the reference's call
    assert torch.equal(m1, mean) and torch.equal(c1, cover)


def test_spline_only_shape_is_the_chamfer_chain(gpu, fx, monkeypatch):
    """Shape b: bit-identical to the minimum of the two one-sided Chamfer distances (the same chain: no tolerance)."""
    from parsenet_codebase_amd.chamfer import chamfer_distance_single_shape
    pts, prm, live = _shape(fx, "b", gpu)
    assert live == ["open-spline", "closed-spline"]
    (_, _, dmin, key), = _run(monkeypatch, "fused", [pts], [prm], return_points=True)
    each = torch.stack([chamfer_distance_single_shape(prm[k][1][0], pts, one_side=True, sqrt=True, reduce=False)
                        for k in (0, 1)], 0)
    want, arg = torch.min(each, 0)
    assert torch.equal(dmin, want)
    assert torch.equal(key, arg) and (key == 0).any() and (key == 1).any()
    assert float(np.abs(dmin.cpu().numpy().astype(np.float64) - fx["b_min32"]).max()) <= max(_bars(fx).values())


def _agree(fx, live, fused, tensor, scale=1.0, extra=None):
    """fused and tensor results of one shape (mean, cover, dmin, key): dmin within the bar of the type that wins the
    point in the fused result (``extra``: the bar of entries that are not in the fixture), the mean within the
    largest bar, the cover equal up to the points within the bar of 0.01."""
    bars = dict(_bars(fx), **(extra or {}))
    d_f, d_t = fused[2].cpu().numpy().astype(np.float64), tensor[2].cpu().numpy().astype(np.float64)
    bar = scale * np.asarray([bars[live[int(k)]] for k in fused[3].cpu().numpy()])
    err = np.abs(d_f - d_t)
    print("max |fused - tensor| / bar = %.3f (max error %.3e)" % ((err / bar).max(), err.max()))
    assert (err <= bar).all()
    assert abs(fused[0].item() - tensor[0].item()) <= scale * max(bars.values())
    near = np.abs(d_t - 0.01) <= bar
    assert np.array_equal((d_f < 0.01)[~near], (d_t < 0.01)[~near])
    assert abs(fused[1].item() - tensor[1].item()) <= near.mean() + 1e-6
    return err


def test_analytic_only_shape_fused_agrees_with_tensor(gpu, fx, monkeypatch):
    pts, prm, live = _shape(fx, "c", gpu)
    fused, = _run(monkeypatch, "fused", [pts], [prm], return_points=True)
    tensor, = _run(monkeypatch, "tensor", [pts], [prm], return_points=True)
    _agree(fx, live, fused, tensor)
    assert float(np.abs(fused[2].cpu().numpy().astype(np.float64) - fx["c_min32"]).max()) <= max(_bars(fx).values())


def test_batch_is_one_launch_and_equals_single_calls(gpu, fx, monkeypatch):
    """The three shapes together (1 237, 300 and 300 points): one launch, the counter rises by 3, every figure bit
    for bit that of the single call; and a single shape with one primitive."""
    from parsenet_codebase_amd import kernels, metrics
    shapes = [_shape(fx, tag, gpu) for tag in "abc"]
    single = [_run(monkeypatch, "fused", [p], [prm], return_points=True)[0] for p, prm, _ in shapes]
    launches = []
    real = kernels.point_primitive_min
    monkeypatch.setattr(kernels, "point_primitive_min", lambda *a, **k: (launches.append(1), real(*a, **k))[1])
    before = metrics.CALLS_PCOVER["fused"]
    batch = _run(monkeypatch, "fused", [p for p, _, _ in shapes], [prm for _, prm, _ in shapes], return_points=True)
    assert len(launches) == 1 and metrics.CALLS_PCOVER["fused"] == before + 3
    for one, many in zip(single, batch):
        assert all(torch.equal(x, y) for x, y in zip(one, many))
    same_n = _run(monkeypatch, "fused", torch.stack([shapes[1][0], shapes[2][0]]), [shapes[1][1], shapes[2][1]])
    assert all(torch.equal(x, y) for b in (0, 1) for x, y in zip(same_n[b], single[1 + b][:2]))   # a (B,N,3) tensor
    pts, prm, _ = shapes[2]
    sphere = {5: prm[1]}
    fused, = _run(monkeypatch, "fused", [pts], [sphere], return_points=True)
    tensor, = _run(monkeypatch, "tensor", [pts], [sphere], return_points=True)
    assert (fused[3] == 5).all()
    _agree(fx, {5: "sphere"}, fused, tensor)


def test_torus_entry_is_merged_after_the_launch(gpu, fx, monkeypatch):
    """A torus has no slot in the kernel: the tensor expression is merged in.  Where the torus wins, both paths hold
    the same torus value, so they differ by at most the error of the runner-up: the largest bar."""
    pts, prm, live = _shape(fx, "c", gpu)
    torus = ["torus", torch.tensor([0.1, -0.2, 1.0], device=gpu), torch.tensor([-0.25, -0.25, 0.1], device=gpu),
             torch.tensor(0.12, device=gpu), torch.tensor(0.04, device=gpu)]
    prm = {0: prm[0], 1: torus, 2: prm[1], 3: prm[2], 4: None, 5: prm[3]}
    live = {0: "plane", 1: "torus", 2: "sphere", 3: "cylinder", 5: "cone"}
    fused, = _run(monkeypatch, "fused", [pts], [prm], return_points=True)
    tensor, = _run(monkeypatch, "tensor", [pts], [prm], return_points=True)
    assert (fused[3] == 1).any() and (fused[3] != 1).any()
    _agree(fx, live, fused, tensor, extra={"torus": max(_bars(fx).values())})
    only = {7: torus}                                                    # no kernel primitive at all
    f1, = _run(monkeypatch, "fused", [pts], [only], return_points=True)
    t1, = _run(monkeypatch, "tensor", [pts], [only], return_points=True)
    assert torch.equal(f1[2], t1[2]) and (f1[3] == 7).all()


def test_evaluation_p_coverage_on_fitted_parameters(gpu, fx, monkeypatch):
    """Evaluation.p_coverage on the parameters the evaluation mode fits for the synthetic shape of
    tests/test_fitting_eval_gpu.py (an open and a closed spline segment among analytic ones): both paths agree.  The
    bars were measured in the unit box (|coordinate| <= 0.5); an fp32 distance error grows with the coordinates, so
    they are scaled by max |coordinate| / 0.5, or by the largest analytic parameter (1 in the fixture), where larger."""
    from tests.test_fitting_eval_gpu import _setup
    torch.cuda.set_device(gpu)
    ev, emb, pts, nrm, lab, prim, logp = _setup(gpu, (21,))
    ev.batched = False                                                   # segment by segment: residual_eval_mode
    np.random.seed(7)
    _, (params, _, _) = ev.fitting_loss(emb, pts, nrm, lab, prim, logp, quantile=0.025, iterations=10, lamb=0.1,
                                        eval=True)
    live = {k: v[0] for k, v in params.items() if v is not None}
    assert any("spline" in n for n in live.values()) and any("spline" not in n for n in live.values())
    biggest = max(float(torch.as_tensor(x).abs().max()) for v in params.values() if v is not None and "spline" not in v[0]
                  for x in v[1:])
    scale = max(1.0, float(pts.abs().max()) / 0.5, biggest / 1.0)       # (the fixture's largest parameter: unit axes)
    # The synthetic shapes are normalised to about the unit box and a sound fit keeps its centres and radii inside a
    # few box widths: a scale above 4 means a degenerate fit (a near-flat sphere or cylinder with a far centre), and
    # the scaled bars would no longer say anything.
    print("scale of the bars: %.3f (largest |coordinate| %.3f, largest analytic parameter %.3f)"
          % (scale, float(pts.abs().max()), biggest))
    assert scale <= 4.0
    out = {}
    for path in ("fused", "tensor"):
        monkeypatch.setenv("PARSENET_PCOVER", path)
        mean, cover = ev.p_coverage(pts[0], params)
        assert mean.dim() == 0 and 0.0 <= cover.item() <= 1.0 and np.isfinite(mean.item())
        out[path] = (mean, cover)
    fused, = _run(monkeypatch, "fused", [pts[0]], [params], return_points=True)
    tensor, = _run(monkeypatch, "tensor", [pts[0]], [params], return_points=True)
    assert torch.equal(fused[0], out["fused"][0]) and torch.equal(tensor[1], out["tensor"][1])
    _agree(fx, live, fused, tensor, scale=scale)
