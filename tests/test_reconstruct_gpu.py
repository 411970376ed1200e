"""GPU: the reconstruction metrics of a batch of shapes (fitting_eval.reconstruct_batch, test.py:108-185): the
coverage reduction of csrc/chamfer.hip against numpy float64 and the tensor library, metrics.coverage_metrics_batch
against coverage_metrics, the batch against the shape-by-shape loop under the same seeds, the trimmed surfaces of
the LS refit, independence of the batch composition, and a shape whose sampling fails."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 0.1
_CACHE = {}


# ---------------------------------------------------------------------------------------------
# 1. the reduction
# ---------------------------------------------------------------------------------------------
def _crafted(rng, n):
    """n squared distances: 0, values under the clamp, the fp32 squares of the floats next to 0.01f and 0.02f on both
    sides, the rest spread over both thresholds."""
    special = [0.0, 1e-6, 9.9e-6, 1e-5]
    for t in (np.float32(0.01), np.float32(0.02)):
        for r in (np.nextafter(t, np.float32(0)), t, np.nextafter(t, np.float32(1))):
            special += [r * r, np.nextafter(r * r, np.float32(0)), np.nextafter(r * r, np.float32(1))]
    x = (rng.uniform(0.0, 0.03, n).astype(np.float32)) ** 2
    k = min(n, len(special))
    pick = rng.permutation(len(special))[:k]
    x[:k] = np.asarray(special, np.float32)[pick]
    return x.astype(np.float32)


def test_coverage_reduce_against_numpy_float64(gpu):
    from parsenet_codebase_amd import kernels as K
    torch.cuda.set_device(gpu)
    rng = np.random.RandomState(11)
    sizes = [(1, 63), (64, 65), (257, 1000)]          # partial wave, exact wave, a wave and one, two strides, four
    shapes = [(_crafted(rng, na), _crafted(rng, nb)) for na, nb in sizes]

    def run(order):
        a = torch.from_numpy(np.concatenate([shapes[i][0] for i in order])).to(gpu)
        b = torch.from_numpy(np.concatenate([shapes[i][1] for i in order])).to(gpu)
        oa = np.concatenate([[0], np.cumsum([sizes[i][0] for i in order])]).astype(np.int32)
        ob = np.concatenate([[0], np.cumsum([sizes[i][1] for i in order])]).astype(np.int32)
        out = K.coverage_reduce(a, torch.from_numpy(oa).to(gpu), b, torch.from_numpy(ob).to(gpu))
        assert out.dtype == torch.float64 and tuple(out.shape) == (len(order), 6)
        return out.cpu().numpy(), (a, oa), (b, ob)

    order = [0, 1, 2]
    got, sa, sb = run(order)
    for k, i in enumerate(order):
        for side, (x, off) in enumerate((sa, sb)):
            seg = x[off[k]:off[k + 1]]
            root = torch.sqrt(torch.clamp(seg, min=1e-5))
            want1, want2 = int((root < 0.01).sum().item()), int((root < 0.02).sum().item())
            host = np.sqrt(np.maximum(shapes[i][side], np.float32(1e-5)))
            assert host.dtype == np.float32 and np.array_equal(root.cpu().numpy(), host)
            total = host.astype(np.float64).sum()
            row = got[k, 3 * side:3 * side + 3]
            print("shape %d side %d: n %d, sum %.17g (numpy %.17g), counts %d %d (tensor library %d %d)"
                  % (i, side, seg.shape[0], row[0], total, row[1], row[2], want1, want2))
            assert row[1] == want1 and row[2] == want2
            assert abs(row[0] - total) <= 1e-12 * total
            assert 0 < want2 or seg.shape[0] == 1
    assert got[2, 1] < got[2, 2] < sizes[2][0]                  # both thresholds cut through the values
    again, _, _ = run([2, 0, 1])                                # the last shape first: the same bits
    assert np.array_equal(again[0].view(np.int64), got[2].view(np.int64))
    assert np.array_equal(again[1].view(np.int64), got[0].view(np.int64))
    assert np.array_equal(again[2].view(np.int64), got[1].view(np.int64))


# ---------------------------------------------------------------------------------------------
# 2. coverage_metrics_batch
# ---------------------------------------------------------------------------------------------
def test_coverage_metrics_batch_equals_coverage_metrics(gpu):
    """Shares: the same counts (coverage_metrics reports an fp32 mean of 0/1 values: count / n to 1e-7 relative);
    means and cd: 2e-6 relative — the fp32 torch.mean of <= 10^4 terms carries about log2(n) 2^-24 = 8e-7."""
    from parsenet_codebase_amd import metrics
    torch.cuda.set_device(gpu)
    rng = np.random.RandomState(4)
    pairs = []
    for m, n in [(700, 500), (333, 901), (257, 640)]:
        pts = rng.uniform(-0.5, 0.5, (n, 3)).astype(np.float32)
        pred = (pts[rng.randint(0, n, m)] + rng.normal(0, 0.008, (m, 3))).astype(np.float32)
        pairs.append((torch.from_numpy(pred).to(gpu), torch.from_numpy(pts).to(gpu)))
    got = metrics.coverage_metrics_batch([p for p, _ in pairs], [q for _, q in pairs])
    for s, (pred, pts) in enumerate(pairs):
        want = metrics.coverage_metrics(pred, pts)
        print("shape %d: batch %s\n         single %s" % (s, got[s], want))
        assert sorted(got[s]) == sorted(want)
        for key, size in (("sk_1", pts.shape[0]), ("sk_2", pts.shape[0]), ("pk_1", pred.shape[0]), ("pk_2", pred.shape[0])):
            count = int(round(want[key] * size))
            assert abs(want[key] * size - count) < 1e-2 and got[s][key] == count / size, key
        for key in ("sk", "pk", "cd"):
            assert abs(got[s][key] - want[key]) <= 2e-6 * abs(want[key]), key
        assert 0 < got[s]["pk_1"] < got[s]["pk_2"] <= 1 and 0 < got[s]["sk_1"] < 1
    alone = metrics.coverage_metrics_batch([pairs[2][0].cpu().numpy()], [pairs[2][1].cpu().numpy()])[0]
    assert alone == got[2]                                      # arrays or tensors, alone or last of three


# ---------------------------------------------------------------------------------------------
# shapes, the loop and the batch (computed once per configuration)
# ---------------------------------------------------------------------------------------------
def _shapes(gpu, ids):
    if ("shapes", ids) not in _CACHE:
        from parsenet_codebase_amd import metrics
        from tests.test_fitting_eval_gpu import _setup
        ev, _, pts, nrm, lab, prim, _ = _setup(gpu, ids)
        cid = np.stack([metrics.continuous_labels(l) for l in lab])
        _CACHE[("shapes", ids)] = (ev, pts, nrm, lab, cid, prim, [100 + i for i in ids])
    return _CACHE[("shapes", ids)]


def _with_plane_draws(ev):
    """residual_eval_mode WITHOUT sample_points does not call sample_plane; under the random-number contract a plane
    takes two draws.  Wrap the fitter so that the reference call consumes them where sample_plane would."""
    orig = ev.fitter.forward_pass_plane

    def wrapped(*a, **kw):
        out = orig(*a, **kw)
        np.random.random()
        np.random.random()
        return out
    ev.fitter.forward_pass_plane = wrapped
    return orig


def _loop(gpu, ids):
    """test.py's loop, shape by shape, on the per-segment entry."""
    if ("loop", ids) not in _CACHE:
        from parsenet_codebase_amd import metrics
        from parsenet_codebase_amd.fitting import SIOU_matched_segments, to_one_hot
        from src.segment_utils import sample_from_collection_of_mesh
        ev, pts, nrm, lab, cid, prim, seeds = _shapes(gpu, ids)
        out = []
        for b in range(len(ids)):
            w = to_one_hot(cid[b], int(cid[b].max()) + 1, device_id=gpu.index)
            np.random.seed(seeds[b])
            with torch.no_grad():
                _, params, surfaces = ev.residual_eval_mode(pts[b], nrm[b], lab[b], cid[b].copy(), prim[b], prim[b], w.T,
                                                            0.01, sample_points=True, if_visualize=True, epsilon=EPS)
            params = dict(params)
            sampled = sample_from_collection_of_mesh(surfaces)
            m = metrics.coverage_metrics(torch.from_numpy(sampled).to(gpu), pts[b])
            m["s_iou"], m["p_iou"] = SIOU_matched_segments(lab[b], cid[b], prim[b], prim[b], w)[:2]
            out.append({"parameters": params, "surfaces": surfaces, "samples": sampled, "metrics": m})
        _CACHE[("loop", ids)] = out
    return _CACHE[("loop", ids)]


def _batch(gpu, ids, if_optimize=False, epsilon=EPS):
    if ("batch", ids, if_optimize, epsilon) not in _CACHE:
        from parsenet_codebase_amd import fitting_eval as FE, surface
        ev, pts, nrm, lab, cid, prim, seeds = _shapes(gpu, ids)
        np.random.seed(77)
        state = np.random.get_state()
        c0, o0 = dict(FE.CALLS_RECONSTRUCT), sum(surface.CALLS_OCCUPANCY.values())
        recs = ev.reconstruct_batch(pts, nrm, lab, cid, prim, prim, seeds, if_optimize=if_optimize, epsilon=epsilon)
        delta = {k: FE.CALLS_RECONSTRUCT[k] - c0[k] for k in c0}
        delta["occupancy_calls"] = sum(surface.CALLS_OCCUPANCY.values()) - o0
        after = np.random.get_state()
        assert np.array_equal(after[1], state[1]) and after[2:] == state[2:]          # the caller's stream is untouched
        _CACHE[("batch", ids, if_optimize, epsilon)] = (recs, delta)
    return _CACHE[("batch", ids, if_optimize, epsilon)]


def _segments(gpu, ids, b, params):
    """Per surface (the fitted segments in the dict's order): key, type, member indices."""
    ev, pts, nrm, lab, cid, prim, seeds = _shapes(gpu, ids)
    out = []
    for key, v in params.items():
        if v is None:
            continue
        idx = np.flatnonzero(cid[b] == key)
        out.append((key, int(np.bincount(prim[b][idx].astype(np.int64)).argmax()), idx))
    return out


def _cloud(gpu, ids, b, seg_type, idx):
    from parsenet_codebase_amd import surface
    from parsenet_codebase_amd.fitting import up_sample_points_torch_memory_efficient
    pts = _shapes(gpu, ids)[1]
    return up_sample_points_torch_memory_efficient(pts[b][torch.from_numpy(idx).to(gpu)], surface._TRIM[seg_type][0])


def _compare(gpu, ids, b, want, got, eps):
    """``got`` against ``want`` (two evaluations of shape b of ``ids``) the way test 3 asks.  Returns True when every
    grid and mask is bit-identical."""
    pw, pg = want["parameters"], got["parameters"]
    assert list(pw) == list(pg)
    assert [None if v is None else v[0] for v in pw.values()] == [None if v is None else v[0] for v in pg.values()]
    segs = _segments(gpu, ids, b, pw)
    assert len(want["surfaces"]) == len(got["surfaces"]) == len(segs) > 0
    excused_total = differ_total = 0
    identical = True
    for (key, seg_type, idx), sw, sg in zip(segs, want["surfaces"], got["surfaces"]):
        assert (sw.size_u, sw.size_v) == (sg.size_u, sg.size_v), key
        spline = "spline" in pw[key][0]
        vtol = (2e-4 if spline else 2e-5) * max(1.0, float(np.abs(sw.vertices).max()))
        dv = float(np.abs(sw.vertices - sg.vertices).max())
        assert dv <= vtol, (key, pw[key][0], dv)
        # cells whose centre distance (float64, the first evaluation's grid and the segment's up-sampled cloud) lies
        # within the vertex tolerance of the threshold: only those may differ, and at most 1 % of the surface's cells
        g = torch.from_numpy(sw.vertices).to(gpu).double().reshape(sw.size_u, sw.size_v, 3)
        cen = ((g[:-1, :-1] + g[:-1, 1:] + g[1:, :-1] + g[1:, 1:]) * 0.25).reshape(-1, 3)
        cloud = _cloud(gpu, ids, b, seg_type, idx).double()
        near = torch.cat([torch.cdist(cen[o:o + 2048], cloud).min(1)[0] for o in range(0, cen.shape[0], 2048)])
        excused = ((near - eps).abs() <= vtol).cpu().numpy()
        differ = sw.mask.reshape(-1) != sg.mask.reshape(-1)
        print("shape %d segment %d (%s): max vertex difference %.3e (granted %.1e), %d cells, %d near the threshold, "
              "%d differ" % (b, key, pw[key][0], dv, vtol, excused.size, excused.sum(), differ.sum()))
        assert excused.mean() < 0.01, key
        assert not (differ & ~excused).any(), key
        excused_total += int(excused.sum())
        differ_total += int(differ.sum())
        identical &= dv == 0.0 and not differ.any()
    mw, mg = want["metrics"], got["metrics"]
    assert mg["s_iou"] == mw["s_iou"] and mg["p_iou"] == mw["p_iou"]
    print("shape %d: first  %s\n         second %s" % (b, mw, mg))
    n = _shapes(gpu, ids)[1][b].shape[0]
    if differ_total == 0:
        assert got["samples"].shape[0] == want["samples"].shape[0]
        for key, size in (("sk_1", n), ("sk_2", n), ("pk_1", got["samples"].shape[0]), ("pk_2", got["samples"].shape[0])):
            assert abs(mg[key] - mw[key]) * size < 1e-2, key               # the same counts
        for key in ("sk", "pk", "cd"):
            print("  %s: relative difference %.3e" % (key, abs(mg[key] - mw[key]) / abs(mw[key])))
            assert abs(mg[key] - mw[key]) <= 2e-6 * abs(mw[key]), key
    else:
        # a differing cell changes the areas, with them the counts per surface and so EVERY later draw: the two sample
        # sets are different samples of (nearly) the same surfaces.  Every sample lies within eps + a cell diagonal
        # of the cloud, every cloud point's distance changes by at most the same: that is the gap a sample can move by
        diag = max(float(np.linalg.norm(np.diff(s.vertices.reshape(s.size_u, s.size_v, 3), axis=0), axis=2).max() +
                         np.linalg.norm(np.diff(s.vertices.reshape(s.size_u, s.size_v, 3), axis=1), axis=2).max())
                   for s in want["surfaces"])
        for key in ("sk", "pk", "cd"):
            assert abs(mg[key] - mw[key]) <= eps + diag, key
    return identical


# ---------------------------------------------------------------------------------------------
# 3. the batch against the loop
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ids", [(3, 21), (21,)])
def test_batch_equals_the_shape_by_shape_loop(gpu, ids):
    """Shapes 3 and 21 instead of 3 and 11: in the loop's own output the closed-spline segment of shape 11 has 11 of
    its 870 cells (1.26 %) within the granted 2e-4 of the threshold, more than the 1 % an excused share may reach, so
    the cap cannot be relied on there (its masks were nevertheless equal, 0 cells differing); shapes 3 and 21 have at
    most 5 of 870.  Observed on an MI355X: every grid bit-identical to the loop's, no cell differing; relative
    differences of sk / pk / cd 8.4e-8 / 4.8e-9 / 3.2e-8 (shape 3) and 4.7e-8 / 3.6e-8 / 6.0e-9 (shape 21) — the fp32
    torch.mean of the loop against the fp64 sums of the batch."""
    torch.cuda.set_device(gpu)
    loop = _loop(gpu, ids)
    recs, delta = _batch(gpu, ids)
    assert delta["shapes"] == len(ids) and delta["occupancy_launches"] == 1 and delta["occupancy_calls"] == 1
    kinds = {v[0] for r in recs for v in r["parameters"].values() if v is not None}
    # the kept counts of the spline stage, the stage's download, the points (cones and cylinders are trimmed by them),
    # masks, areas, the coverage table
    expect = 4 + int(any("spline" in k for k in kinds)) + int(bool(kinds & {"cone", "cylinder"}))
    assert delta["downloads"] == expect, (delta, kinds)
    for b in range(len(ids)):
        got = dict(recs[b])
        assert got["message"] is None and got["samples"].is_cuda and got["samples"].dtype == torch.float32
        _compare(gpu, ids, b, loop[b], got, EPS)


# ---------------------------------------------------------------------------------------------
# 4. the trimmed surfaces of the refit
# ---------------------------------------------------------------------------------------------
def test_refit_surfaces_of_the_batched_entry(gpu):
    from parsenet_codebase_amd import surface
    from parsenet_codebase_amd.fitting import to_one_hot
    torch.cuda.set_device(gpu)
    ids = (21,)
    ev, pts, nrm, lab, cid, prim, seeds = _shapes(gpu, ids)
    w = to_one_hot(cid[0], int(cid[0].max()) + 1, device_id=gpu.index).T
    with pytest.raises(NotImplementedError, match="if_optimize"):
        ev.residual_eval_mode(pts[0], nrm[0], lab[0], cid[0].copy(), prim[0], prim[0], w, 0.01, sample_points=True,
                              if_optimize=True, if_visualize=True)
    recs, _ = _batch(gpu, ids, if_optimize=True, epsilon=None)
    rec = recs[0]
    orig = _with_plane_draws(ev)
    try:
        np.random.seed(seeds[0])
        with torch.no_grad():
            _, params, _ = ev.residual_eval_mode(pts[0], nrm[0], lab[0], cid[0].copy(), prim[0], prim[0], w, 0.01,
                                                 if_optimize=True, if_visualize=True)
    finally:
        ev.fitter.forward_pass_plane = orig
    segs = _segments(gpu, ids, 0, rec["parameters"])
    assert len(segs) == len(rec["surfaces"])
    seen = set()
    for (key, seg_type, idx), s in zip(segs, rec["surfaces"]):
        v = rec["parameters"][key]
        if "spline" not in v[0]:
            continue
        seen.add(v[0])
        grid = v[1][0].cpu().numpy()
        assert (s.size_u, s.size_v) == ((30, 30) if v[0] == "open-spline" else (31, 30))
        assert np.array_equal(s.vertices, grid), key                 # the surface IS the refit's sample grid
        c = params[key][1][0].cpu().numpy()
        d = float(np.abs(grid - c).max())
        print("segment %d (%s): max difference to the per-segment refit %.3e" % (key, v[0], d))
        assert d <= 1e-4 * max(1.0, float(np.abs(c).max())), key
        one = surface.bit_mapping_points_torch(_cloud(gpu, ids, 0, seg_type, idx), grid, surface._TRIM[seg_type][1],
                                               s.size_u, s.size_v)
        assert np.array_equal(one.mask, s.mask), key
    assert seen == {"open-spline", "closed-spline"}
    m = rec["metrics"]
    print("refit metrics", m)
    assert all(np.isfinite(float(x)) for x in m.values()) and m["cd"] == (m["sk"] + m["pk"]) / 2


# ---------------------------------------------------------------------------------------------
# 5. the batch a shape is evaluated in
# ---------------------------------------------------------------------------------------------
def _assert_same_shape(gpu, alone, other, what):
    """Shape 21 alone against the same shape in another batch: identical grids and masks, bit-identical samples, an
    identical metrics row (the SplineNet runs segment by segment on this entry, so that the fitting launches of a
    larger batch do not move a grid in its last bits)."""
    identical = _compare(gpu, (21,), 0, alone, other, EPS)
    print("%s: grids and masks %s" % (what, "bit-identical" if identical else "differ in the last bits"))
    assert identical
    assert torch.equal(alone["samples"], other["samples"])
    assert alone["metrics"] == other["metrics"]


def test_a_shape_does_not_depend_on_its_batch(gpu):
    torch.cuda.set_device(gpu)
    alone = _batch(gpu, (21,))[0][0]
    pair = _shapes(gpu, (3, 21))
    assert torch.equal(pair[1][1], _shapes(gpu, (21,))[1][0]) and pair[6][1] == _shapes(gpu, (21,))[6][0]
    _assert_same_shape(gpu, alone, _batch(gpu, (3, 21))[0][1], "second of (3, 21)")


# ---------------------------------------------------------------------------------------------
# 6. a shape without a surviving surface
# ---------------------------------------------------------------------------------------------
def test_a_shape_whose_sampling_fails_does_not_abort_the_batch(gpu):
    """19 points per segment: every fit is None, no surface, nothing to sample -> metrics None and the message; the
    other shape of the (ragged: lists of (N_b,3)) batch is what it is alone."""
    from parsenet_codebase_amd import fitting_eval as FE
    torch.cuda.set_device(gpu)
    ev, pts, nrm, lab, cid, prim, seeds = _shapes(gpu, (21,))
    rng = np.random.RandomState(2)
    small = rng.uniform(-0.5, 0.5, (57, 3)).astype(np.float32)
    small_n = np.tile(np.asarray([0, 0, 1], np.float32), (57, 1))
    small_l = np.repeat(np.arange(3), 19)
    before = FE.CALLS_RECONSTRUCT["occupancy_launches"]
    recs = ev.reconstruct_batch([pts[0], small], [nrm[0], small_n], [lab[0], small_l], [cid[0], small_l],
                                [prim[0], np.ones(57, np.int64)], [prim[0], np.ones(57, np.int64)], [seeds[0], 5],
                                epsilon=EPS)
    assert FE.CALLS_RECONSTRUCT["occupancy_launches"] == before + 1
    bad = recs[1]
    assert bad["metrics"] is None and bad["samples"] is None and bad["surfaces"] == []
    assert "no surface with a kept cell" in bad["message"]
    assert list(bad["parameters"].values()) == [None, None, None]
    _assert_same_shape(gpu, _batch(gpu, (21,))[0][0], recs[0], "next to a shape without a surface")
    only = ev.reconstruct_batch([small], [small_n], [small_l], [small_l], [np.ones(57, np.int64)],
                                [np.ones(57, np.int64)], [5])
    assert only[0]["metrics"] is None and only[0]["message"] == bad["message"]
