"""Generate tests/golden/surface.npz by running the REFERENCE's own functions on the CPU:

    python tests/golden/make_golden_surface.py

create_grid, Fit.sample_plane / sample_sphere / sample_cylinder_trim / sample_cone_trim,
up_sample_points_torch_memory_efficient, sample_mesh and triangle_area_multi are the reference's (imported under the
stubs of make_golden.py); the two-triangle tessellation of the kept cells is written out in numpy because open3d is a
stub.  Only DATA is written: inputs, grids, masks, sampled points and the numpy seeds.

One segment per surface type with the real grid sizes, random clouds of 200-400 points (multiples of 100: the
reference's up-sampling only treats whole chunks of 100 points).  The generator ABORTS when an input leaves the
ground the tests stand on:
  * more than 1 % of a segment's cells with a float64 nearest distance within 4e-6 of the threshold;
  * a cone whose trimming is not ring-uniform (whole rings of 51 points);
  * a face pick within 1e-9 of a step of the area cdf.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests.golden.make_golden import install_stubs, save  # noqa: E402

NEAR = 4e-6
SEED_PLANE, SEED_SAMPLE, SEED_ONE = 1234, 4321, 99
NAMES = ["closed", "open", "sphere", "plane", "cone", "cylinder"]
TYPES = {"closed": 0, "open": 2, "sphere": 5, "plane": 1, "cone": 3, "cylinder": 4}
ROUNDS = {"closed": 2, "open": 2, "sphere": 2, "plane": 3, "cone": 3, "cylinder": 3}
THRES = {"closed": 0.06, "open": 0.06, "sphere": 0.03, "plane": 0.02, "cone": 0.03, "cylinder": 0.03}


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def frame(a):
    """two unit vectors orthogonal to the unit vector a and to each other"""
    h = np.array([1.0, 0, 0]) if abs(a[0]) < 0.9 else np.array([0, 1.0, 0])
    u = unit(np.cross(a, h))
    return u, np.cross(a, u)


def nearest_f64(grid32, su, sv, cloud32):
    """float64 distance of every cell centre of the fp32 grid to the nearest point of the fp32 cloud"""
    g = grid32.astype(np.float64).reshape(su, sv, 3)
    c = ((g[:-1, :-1] + g[:-1, 1:] + g[1:, :-1] + g[1:, 1:]) * 0.25).reshape(-1, 3)
    p = cloud32.astype(np.float64)
    out = np.empty(c.shape[0])
    for s in range(0, c.shape[0], 1024):
        d = ((c[s:s + 1024, None, :] - p[None]) ** 2).sum(2)
        out[s:s + 1024] = np.sqrt(d.min(1))
    return out


def tessellate(vertices, su, sv, mask):
    """(v1, v2, v3) of the triangles of the kept cells, tessalate_points_fast's order; float64 like open3d's
    Vector3dVector of the fp32 vertices"""
    v = vertices.astype(np.float64)
    tri = []
    for i in range(su - 1):
        for j in range(sv - 1):
            if mask[i, j]:
                tri.append([i * sv + j, (i + 1) * sv + j, (i + 1) * sv + j + 1])
                tri.append([i * sv + j, (i + 1) * sv + j + 1, i * sv + j + 1])
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    return v[tri[:, 0]], v[tri[:, 1]], v[tri[:, 2]]


def reference_collection(ref_utils, meshes, N):
    """src/segment_utils.py:83-123 on (vertices, su, sv, mask) tuples; open3d's remove_unreferenced_vertices leaves
    vertices[triangles] as it is.  Returns per surviving mesh (n_i, faces, points, picks, cdf) and the areas."""
    new = [m for m in meshes if m[3].any()]
    tris = [tessellate(*m) for m in new]
    A = [np.sum(ref_utils.triangle_area_multi(*t)) for t in tris]
    area = np.sum(A)
    out = []
    for index, (v1, v2, v3) in enumerate(tris):
        n = int((N * A[index]) // area)
        if n > 10:
            state = np.random.get_state()
            points, _, face_ids = ref_utils.sample_mesh(v1, v2, v3, n=n, norms=False)
            after = np.random.get_state()
            np.random.set_state(state)
            picks = np.random.random_sample(n)          # what random.choice drew
            np.random.set_state(after)
            areas = ref_utils.triangle_area_multi(v1, v2, v3)
            areas = areas + np.min(areas) + 1e-10
            cdf = (areas / np.sum(areas)).cumsum()
            cdf /= cdf[-1]
            assert np.array_equal(cdf.searchsorted(picks, side="right"), face_ids)
            gap = np.abs(cdf[None, :] - picks[:, None]).min()
            assert gap > 1e-9, "a face pick within 1e-9 of a cdf step (%g): change the seed" % gap
            out.append((n, face_ids, points))
        else:
            out.append((n, None, None))
    return out, np.asarray(A)


def main():
    install_stubs()
    import src.fitting_utils as ref_fu
    import src.primitive_forward as ref_pf
    import src.utils as ref_utils
    fit = ref_pf.Fit()
    rng = np.random.RandomState(2024)
    arrays = {"names": np.asarray(NAMES), "types": np.asarray([TYPES[n] for n in NAMES]),
              "thres": np.asarray([THRES[n] for n in NAMES]), "rounds": np.asarray([ROUNDS[n] for n in NAMES]),
              "seed_plane": np.asarray(SEED_PLANE), "seed_sample": np.asarray(SEED_SAMPLE),
              "seed_one": np.asarray(SEED_ONE)}
    points, grids, sizes = {}, {}, {}

    # ---- analytic surfaces: parameters as the fits hand them over (float32 arrays, Python floats) ----------------
    n = unit([0.3, -0.5, 0.8]).astype(np.float32)
    d = 0.2
    u, v = frame(n.astype(np.float64))
    uv = rng.uniform(-0.45, 0.45, (300, 2))
    points["plane"] = (d * n + uv[:, 0:1] * u + uv[:, 1:2] * v + 0.002 * rng.randn(300, 3)).astype(np.float32)
    mean = ref_fu.project_to_plane(torch.from_numpy(points["plane"]), torch.from_numpy(n.reshape(1, 3)), d)
    mean = torch.mean(mean, 0).numpy()
    np.random.seed(SEED_PLANE)
    grids["plane"] = fit.sample_plane(d, n.reshape(1, 3), mean)
    sizes["plane"] = (120, 120)
    arrays.update(plane_n=n, plane_d=np.asarray(d), plane_mean=mean)

    r, c = 0.6, np.asarray([0.1, -0.2, 0.05], np.float32)
    q = rng.randn(200, 3)
    q[:, 2] = np.abs(q[:, 2]) * 0.6
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    points["sphere"] = (c + r * q + 0.002 * rng.randn(200, 3)).astype(np.float32)
    grids["sphere"] = fit.sample_sphere(r, c.reshape(1, 3), N=10000)[0]
    sizes["sphere"] = (100, 100)
    arrays.update(sphere_r=np.asarray(r), sphere_c=c)

    r, c, a = 0.3, np.asarray([-0.1, 0.1, 0.0], np.float32), unit([0.2, 0.9, -0.4]).astype(np.float32)
    u, v = frame(a.astype(np.float64))
    ang, h = rng.uniform(0.0, 4.0, 300), rng.uniform(-0.5, 0.5, 300)
    points["cylinder"] = (c + h[:, None] * a + r * (np.cos(ang)[:, None] * u + np.sin(ang)[:, None] * v)
                          + 0.002 * rng.randn(300, 3)).astype(np.float32)
    grids["cylinder"] = fit.sample_cylinder_trim(r, c, a, points["cylinder"], N=10000)[0]
    sizes["cylinder"] = (200, 60)
    arrays.update(cylinder_r=np.asarray(r), cylinder_c=c, cylinder_a=a)

    apex, a, theta = np.asarray([0.0, 0.0, 0.0], np.float32), unit([0.1, 0.2, 0.95]).astype(np.float32), 0.5
    u, v = frame(a.astype(np.float64))
    ang, h = rng.uniform(0.0, 5.0, 400), rng.uniform(0.3, 0.9, 400)
    points["cone"] = (apex + h[:, None] * a + (h * np.tan(theta))[:, None] * (np.cos(ang)[:, None] * u + np.sin(ang)[:, None] * v)
                      + 0.002 * rng.randn(400, 3)).astype(np.float32)
    cone = fit.sample_cone_trim(apex, a, theta, points["cone"])[0]
    assert cone.shape[0] % 51 == 0 and cone.shape[0] >= 2 * 51, cone.shape
    rings = cone.reshape(-1, 51, 3)
    assert np.array_equal(rings[:, 0], rings[:, 50]), "the reference's cone trimming is not ring-uniform here"
    grids["cone"] = cone
    sizes["cone"] = (cone.shape[0] // 51, 51)
    arrays.update(cone_c=apex, cone_a=a, cone_theta=np.asarray(theta))

    # ---- spline samples: data (what a SplineNet hands over, float32) -------------------------------------------
    s, t = np.meshgrid(np.linspace(-0.5, 0.5, 30), np.linspace(-0.5, 0.5, 30), indexing="ij")
    grids["open"] = np.stack([s, t, 0.4 * s * s - 0.3 * t * t + 0.1 * s], 2).reshape(-1, 3).astype(np.float32)
    sizes["open"] = (30, 30)
    st = rng.uniform(-0.5, 0.2, (300, 2))
    points["open"] = (np.stack([st[:, 0], st[:, 1], 0.4 * st[:, 0] ** 2 - 0.3 * st[:, 1] ** 2 + 0.1 * st[:, 0]], 1)
                      + 0.002 * rng.randn(300, 3)).astype(np.float32)
    ang = np.linspace(0, 2 * np.pi, 31)
    ang[-1] = 0.0
    hh = np.linspace(-0.4, 0.4, 30)
    rad = 0.25 + 0.1 * np.cos(3 * hh)
    grids["closed"] = np.stack([np.cos(ang)[:, None] * rad[None], np.sin(ang)[:, None] * rad[None],
                                np.repeat(hh[None], 31, 0)], 2).reshape(-1, 3).astype(np.float32)
    sizes["closed"] = (31, 30)
    an, hp = rng.uniform(0, 2 * np.pi, 300), rng.uniform(-0.4, 0.1, 300)
    rp = 0.25 + 0.1 * np.cos(3 * hp)
    points["closed"] = (np.stack([np.cos(an) * rp, np.sin(an) * rp, hp], 1) + 0.002 * rng.randn(300, 3)).astype(np.float32)

    # ---- occupancy: the reference's create_grid on its own up-sampled clouds ------------------------------------
    meshes = []
    for name in NAMES:
        su, sv = sizes[name]
        up = ref_fu.up_sample_points_torch_memory_efficient(torch.from_numpy(points[name]), ROUNDS[name]).numpy()
        mask = ref_fu.create_grid(up, grids[name], su, sv, thres=THRES[name])[0].numpy().astype(bool)
        g32 = grids[name].astype(np.float32)
        near = np.abs(nearest_f64(g32, su, sv, up.astype(np.float32)) - THRES[name]) <= NEAR
        assert near.mean() <= 0.01, "%s: %.2f %% of the cells within %g of the threshold" % (name, 100 * near.mean(), NEAR)
        assert 0 < mask.sum() < mask.size, name
        print("%-9s grid %3d x %3d, cloud %5d, kept %5d of %5d cells, %d near the threshold"
              % (name, su, sv, up.shape[0], mask.sum(), mask.size, near.sum()))
        arrays.update({name + "_points": points[name], name + "_up": up.astype(np.float32), name + "_grid": g32,
                       name + "_size": np.asarray([su, sv]), name + "_mask": mask})
        meshes.append((g32, su, sv, mask))

    # ---- sampling: the six surfaces + one without a kept cell (dropped) + one whose share stays <= 10 (skipped) --
    empty = (arrays["open_grid"], 30, 30, np.zeros((29, 29), bool))
    tiny_mask = np.zeros((119, 119), bool)
    tiny_mask[5, 7] = True
    tiny = (arrays["plane_grid"], 120, 120, tiny_mask)
    N = 3000
    order = [0, 1, 6, 2, 3, 7, 4, 5]                       # positions of empty (6) and tiny (7) among the six
    coll = [(meshes + [empty, tiny])[i] for i in order]
    np.random.seed(SEED_SAMPLE)
    res, A = reference_collection(ref_utils, coll, N)
    after = np.random.random()
    counts = [r[0] for r in res]
    assert min(counts) <= 10 < max(counts)
    arrays.update(sample_order=np.asarray(order), sample_N=np.asarray(N), sample_area=A,
                  sample_counts=np.asarray(counts), sample_stream_after=np.asarray(after),
                  sample_faces=np.concatenate([r[1] for r in res if r[1] is not None]).astype(np.int32),
                  sample_points=np.concatenate([r[2] for r in res if r[2] is not None]).astype(np.float32),
                  tiny_mask=tiny_mask)
    print("collection: counts", counts, "-> %d points" % arrays["sample_points"].shape[0])
    # a mesh with ONE kept cell, alone: all N points on its two triangles
    np.random.seed(SEED_ONE)
    res, _ = reference_collection(ref_utils, [tiny], 64)
    assert res[0][0] == 64
    arrays.update(one_N=np.asarray(64), one_faces=res[0][1].astype(np.int32), one_points=res[0][2].astype(np.float32))
    save("surface", **arrays)


if __name__ == "__main__":
    main()
