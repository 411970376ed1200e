"""Trimmed surfaces on the GPU: the occupancy kernel of csrc/surface.hip against the ragged Chamfer kernel (bit for
bit) and against the reference's create_grid (fixture tests/golden/surface.npz, written by
tests/golden/make_golden_surface.py), the analytic grids, the area-weighted sampler and the evaluation-mode call of
the reference's test.py end to end."""
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["closed", "open", "sphere", "plane", "cone", "cylinder"]


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(ROOT, "tests", "golden", "surface.npz"), allow_pickle=False)


def _surface_grid(rng, su, sv):
    """a smooth random height field over [-0.5, 0.5]^2 with jittered vertices, fp32, |coordinates| < 2"""
    s, t = np.meshgrid(np.linspace(-0.5, 0.5, su), np.linspace(-0.5, 0.5, sv), indexing="ij")
    a, b, c = rng.uniform(-0.5, 0.5, 3)
    z = a * s * s + b * t * t + c * s * t
    g = np.stack([s, t, z], 2) + rng.uniform(-1e-3, 1e-3, (su, sv, 3))
    return g.reshape(-1, 3).astype(np.float32)


def _cloud_near(rng, grid, n, noise=0.01):
    return (grid[rng.randint(0, grid.shape[0], n)] + noise * rng.randn(n, 3)).astype(np.float32)


def _centres(g, su, sv):
    g = g.reshape(su, sv, 3)
    return ((((g[:-1, :-1] + g[:-1, 1:]) + g[1:, :-1]) + g[1:, 1:]) * 0.25).reshape(-1, 3)


def _chamfer_masks(grids, sizes, clouds, thres, dev):
    """sqrt(min d) < thres by the ragged Chamfer kernel on centres from the pinned tensor expression"""
    from parsenet_codebase_amd import kernels as K
    cen = [_centres(g, u, v) for g, (u, v) in zip(grids, sizes)]
    offa = np.concatenate([[0], np.cumsum([c.shape[0] for c in cen])]).astype(np.int32)
    offb = np.concatenate([[0], np.cumsum([c.shape[0] for c in clouds])]).astype(np.int32)
    minA = K.chamfer_nn_ragged(torch.cat(cen).contiguous(), torch.from_numpy(offa).to(dev), int(np.diff(offa).max()),
                               torch.cat(clouds).contiguous(), torch.from_numpy(offb).to(dev),
                               int(np.diff(offb).max()), True, False)[0]
    root = torch.sqrt(minA)
    return [root[offa[s]:offa[s + 1]] < torch.tensor(np.float32(thres[s]), device=dev) for s in range(len(cen))], root, offa


@pytest.mark.gpu
def test_occupancy_equals_the_chamfer_kernel_bit_for_bit(gpu):
    from parsenet_codebase_amd import surface
    torch.cuda.set_device(gpu)
    rng = np.random.RandomState(5)
    spec = [((2, 2), 1, 0.05), ((3, 5), 63, 0.0), ((30, 30), 64, 0.1), ((31, 30), 65, 1e3), ((120, 120), 1025, 0.02),
            ((120, 120), 4097, 0.03), ((30, 30), 4097, 0.1), ((3, 5), 64, 0.02), ((30, 30), 65, 0.07)]
    grids, sizes, clouds, thres = [], [], [], []
    for (su, sv), n, th in spec:
        g = _surface_grid(rng, su, sv)
        grids.append(g)
        sizes.append((su, sv))
        clouds.append(_cloud_near(rng, g, n))
        thres.append(th)
    clouds[6] = (clouds[6] + np.float32(1.2)).astype(np.float32)          # wholly outside the grid's box
    cen7 = _centres(torch.from_numpy(grids[7]), 3, 5).numpy()
    clouds[7][5] = cen7[3]                                                # a point exactly on a centre
    grids = [torch.from_numpy(g).to(gpu) for g in grids]
    clouds = [torch.from_numpy(c).to(gpu) for c in clouds]
    # segment 8: the threshold IS the nearest distance of cell 100 as floats — strict < rejects the cell
    _, root, offa = _chamfer_masks(grids, sizes, clouds, thres, gpu)
    thres[8] = float(root[offa[8] + 100].item())
    assert thres[8] > 0.0
    want, root, offa = _chamfer_masks(grids, sizes, clouds, thres, gpu)
    before = dict(surface.CALLS_OCCUPANCY)
    got = surface.grid_occupancy(grids, sizes, clouds, thres, kernel="dedicated")
    assert surface.CALLS_OCCUPANCY["dedicated"] == before["dedicated"] + 1
    assert surface.CALLS_OCCUPANCY["chamfer"] == before["chamfer"]
    for s, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == torch.bool and g.shape == (sizes[s][0] - 1, sizes[s][1] - 1)
        assert torch.equal(g.reshape(-1), w), "segment %d: %d cells differ" % (s, int((g.reshape(-1) != w).sum()))
    assert not got[1].any() and got[3].all() and not got[6].any()       # thres 0, keeps everything, outside
    assert got[7].reshape(-1)[3] and 0 < int(got[4].sum()) < got[4].numel() and got[5].any()
    assert not got[8].reshape(-1)[100]
    up = thres[:8] + [float(np.nextafter(np.float32(thres[8]), np.float32(1)))]
    assert surface.grid_occupancy(grids, sizes, clouds, up, kernel="dedicated")[8].reshape(-1)[100]
    # the module's own Chamfer path, and the same batch in another segment order
    for s, m in enumerate(surface.grid_occupancy(grids, sizes, clouds, thres, kernel="chamfer")):
        assert torch.equal(m, got[s])
    order = [5, 0, 8, 3, 1, 7, 2, 6, 4]
    again = surface.grid_occupancy([grids[i] for i in order], [sizes[i] for i in order], [clouds[i] for i in order],
                                   [thres[i] for i in order], kernel="dedicated")
    for k, i in enumerate(order):
        assert torch.equal(again[k], got[i])


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["dedicated", "chamfer"])
def test_occupancy_against_the_reference(gpu, fx, kernel):
    """create_grid's masks on the reference's own up-sampled clouds.  Cells whose float64 nearest distance lies within
    4e-6 of the threshold are excused (coordinates below 2: an ulp of 2.4e-7, four roundings in the centre and a
    handful in the distance), at most 1 % of a segment's cells."""
    from parsenet_codebase_amd import surface
    torch.cuda.set_device(gpu)
    grids = [torch.from_numpy(fx[n + "_grid"]).to(gpu) for n in NAMES]
    clouds = [torch.from_numpy(fx[n + "_up"]).to(gpu) for n in NAMES]
    sizes = [tuple(int(v) for v in fx[n + "_size"]) for n in NAMES]
    thres = [float(t) for t in fx["thres"]]
    got = surface.grid_occupancy(grids, sizes, clouds, thres, kernel=kernel)
    for s, n in enumerate(NAMES):
        su, sv = sizes[s]
        g = grids[s].double().reshape(su, sv, 3)
        cen = ((g[:-1, :-1] + g[:-1, 1:] + g[1:, :-1] + g[1:, 1:]) * 0.25).reshape(-1, 3)
        near = torch.cat([torch.cdist(cen[o:o + 2048], clouds[s].double()).min(1)[0] for o in range(0, cen.shape[0], 2048)])
        excused = ((near - thres[s]).abs() <= 4e-6).cpu().numpy()
        assert excused.mean() <= 0.01, n
        bad = (got[s].reshape(-1).cpu().numpy() != fx[n + "_mask"].reshape(-1)) & ~excused
        print("%s: %d cells, %d excused, %d differ" % (n, excused.size, excused.sum(), bad.sum()))
        assert not bad.any(), n


def test_grids_match_the_reference(fx):
    """float64 grids of the analytic surfaces, compared after the cast to fp32: 1e-5 absolute on unit-scale shapes.
    (Host arithmetic: runs without a GPU.)"""
    from parsenet_codebase_amd import surface as S
    np.random.seed(int(fx["seed_plane"]))
    got = {"plane": S.sample_plane(float(fx["plane_d"]), fx["plane_n"].reshape(1, 3), fx["plane_mean"]),
           "sphere": S.sample_sphere(float(fx["sphere_r"]), fx["sphere_c"].reshape(1, 3)),
           "cylinder": S.sample_cylinder_trim(float(fx["cylinder_r"]), fx["cylinder_c"], fx["cylinder_a"],
                                              fx["cylinder_points"]),
           "cone": S.sample_cone_trim(fx["cone_c"], fx["cone_a"], float(fx["cone_theta"]), fx["cone_points"])}
    for name, g in got.items():
        su, sv = (int(v) for v in fx[name + "_size"])
        assert g.dtype == np.float64 and g.shape == (su * sv, 3), name
        assert np.abs(g.astype(np.float32) - fx[name + "_grid"]).max() <= 1e-5, name
    assert got["cone"].shape[0] % 51 == 0


def _collection(fx):
    from parsenet_codebase_amd.surface import TrimmedSurface
    six = [TrimmedSurface(fx[n + "_grid"], *fx[n + "_size"], fx[n + "_mask"]) for n in NAMES]
    empty = TrimmedSurface(fx["open_grid"], 30, 30, np.zeros((29, 29), bool))
    tiny = TrimmedSurface(fx["plane_grid"], 120, 120, fx["tiny_mask"])
    return [(six + [empty, tiny])[i] for i in fx["sample_order"]], tiny


@pytest.mark.gpu
def test_sampling_against_the_reference(gpu, fx):
    """The reference's masks, the fixture's seed: the same faces, points to 1e-6, the same count; a surface without
    a kept cell is dropped, one whose share stays at 10 points or fewer is skipped, and a surface with a single kept
    cell is sampled on its two triangles."""
    from src.segment_utils import sample_from_collection_of_mesh
    torch.cuda.set_device(gpu)
    coll, tiny = _collection(fx)
    np.random.seed(int(fx["seed_sample"]))
    pts, faces = sample_from_collection_of_mesh(coll, N=int(fx["sample_N"]), return_faces=True)
    assert np.random.random() == float(fx["sample_stream_after"])
    assert pts.dtype == np.float32 and pts.shape == fx["sample_points"].shape
    assert [f.shape[0] for f in faces] == [int(k) for k in fx["sample_counts"] if k > 10]
    assert np.array_equal(np.concatenate(faces), fx["sample_faces"])
    assert np.abs(pts - fx["sample_points"]).max() <= 1e-6
    np.random.seed(int(fx["seed_sample"]))
    assert np.array_equal(sample_from_collection_of_mesh(coll, N=int(fx["sample_N"])), pts)
    np.random.seed(int(fx["seed_one"]))
    pts, faces = sample_from_collection_of_mesh([tiny], N=int(fx["one_N"]), return_faces=True)
    assert np.array_equal(faces[0], fx["one_faces"]) and set(faces[0].tolist()) == {0, 1}
    assert np.abs(pts - fx["one_points"]).max() <= 1e-6
    with pytest.raises(ValueError):
        sample_from_collection_of_mesh([coll[2]], N=100)                  # nothing but a surface without a kept cell


def _shape(rng, n=500):
    """~2000 points: a plane patch, a sphere cap, a cylinder part and a saddle (open spline), apart from each other"""
    uv = rng.uniform(-0.3, 0.3, (n, 2))
    plane = np.stack([uv[:, 0] - 0.6, uv[:, 1], np.full(n, -0.4)], 1)
    plane_n = np.tile([0.0, 0.0, 1.0], (n, 1))
    q = rng.randn(n, 3)
    q[:, 2] = np.abs(q[:, 2])
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    sphere = np.array([0.5, 0.5, 0.0]) + 0.3 * q
    ang, h = rng.uniform(0, 2 * np.pi, n), rng.uniform(-0.3, 0.3, n)
    ring = np.stack([np.cos(ang), np.sin(ang), np.zeros(n)], 1)
    cyl = np.array([0.5, -0.5, 0.0]) + 0.2 * ring + h[:, None] * np.array([0, 0, 1.0])
    st = rng.uniform(-0.3, 0.3, (n, 2))
    saddle = np.stack([st[:, 0] - 0.5, st[:, 1] + 0.1, 0.5 + st[:, 0] ** 2 - st[:, 1] ** 2], 1)
    saddle_n = np.stack([-2 * st[:, 0], 2 * st[:, 1], np.ones(n)], 1)
    saddle_n /= np.linalg.norm(saddle_n, axis=1, keepdims=True)
    pts = np.concatenate([plane, sphere, cyl, saddle]).astype(np.float32)
    nrm = np.concatenate([plane_n, q, ring, saddle_n]).astype(np.float32)
    lab = np.repeat(np.arange(4), n).astype(np.int32)
    prim = np.repeat([1, 5, 4, 2], n).astype(np.int32)
    return pts, nrm, lab, prim


@pytest.mark.gpu
def test_evaluation_mode_end_to_end(gpu, monkeypatch):
    """test.py:126-168: residual_eval_mode(sample_points=True, if_visualize=True, epsilon=0.1) -> trimmed surfaces
    -> 10 000 samples -> coverage metrics.  p_k stays below epsilon + the largest cell diagonal: every kept centre
    has a cloud point within epsilon and every sample lies within a cell diagonal of its kept centre."""
    from parsenet_codebase_amd import metrics, surface
    from src.model import DGCNNControlPoints
    from src.residual_utils import Evaluation
    from src.segment_utils import sample_from_collection_of_mesh
    from tests.golden.common import deterministic_init
    torch.cuda.set_device(gpu)
    pts, nrm, lab, prim = _shape(np.random.RandomState(3))
    ev = Evaluation(closed_path=deterministic_init(DGCNNControlPoints(20, num_points=10, mode=1), salt=1),
                    open_path=deterministic_init(DGCNNControlPoints(20, num_points=10, mode=0)))
    P, Nr = torch.from_numpy(pts).to(gpu), torch.from_numpy(nrm).to(gpu)
    w = torch.nn.functional.one_hot(torch.from_numpy(lab).long(), 4).float().t().to(gpu)
    eps = 0.1

    def run(**kw):
        np.random.seed(17)
        with torch.no_grad():
            return ev.residual_eval_mode(P, Nr, lab, lab.copy(), prim, prim, w, 0.01, sample_points=True,
                                         if_visualize=True, epsilon=eps, **kw)

    results = {}
    for name in ("dedicated", "chamfer"):
        monkeypatch.setenv("PARSENET_TRIM_KERNEL", name)
        before = dict(surface.CALLS_OCCUPANCY)
        results[name] = run()
        assert surface.CALLS_OCCUPANCY[name] == before[name] + 1             # one launch for the shape
    loss, params, surfaces = results["dedicated"]
    assert loss == []
    kinds = sorted(v[0] for v in params.values() if v is not None)
    assert kinds == ["cylinder", "open-spline", "plane", "sphere"]
    assert len(surfaces) == len(kinds) and all(isinstance(s, surface.TrimmedSurface) for s in surfaces)
    assert sorted((s.size_u, s.size_v) for s in surfaces) == [(30, 30), (100, 100), (120, 120), (200, 60)]
    for a, b in zip(surfaces, results["chamfer"][2]):
        assert np.array_equal(a.vertices, b.vertices) and np.array_equal(a.mask, b.mask)
    assert sum(int(s.mask.any()) for s in surfaces) >= 3                     # the analytic fits cover their points
    np.random.seed(18)
    sampled = sample_from_collection_of_mesh(surfaces)
    assert sampled.dtype == np.float32 and 9900 < sampled.shape[0] <= 10000
    m = metrics.coverage_metrics(torch.from_numpy(sampled).to(gpu), P)
    assert all(np.isfinite(v) for v in m.values()), m
    diag = 0.0
    for s in surfaces:
        g = s.vertices.astype(np.float64).reshape(s.size_u, s.size_v, 3)
        d1 = np.linalg.norm(g[:-1, :-1] - g[1:, 1:], axis=2)
        d2 = np.linalg.norm(g[:-1, 1:] - g[1:, :-1], axis=2)
        if s.mask.any():
            diag = max(diag, float(np.maximum(d1, d2).max()))
    print("coverage", m, "largest cell diagonal %.4f" % diag)
    assert m["pk"] < eps + diag
    with pytest.raises(NotImplementedError, match="if_optimize"):
        run(if_optimize=True)
