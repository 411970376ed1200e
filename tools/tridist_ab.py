"""A/B of the exact point-to-surface distance (csrc/tridist.hip) with pruning on and off, and the first measurement of
what the sampling costs the coverage figure: sk_1 / sk against 10 000 samples beside p_cover_surface / p_dist_surface
against the surfaces themselves, on the same shapes.

    python tools/tridist_ab.py [--out profiles/tridist_ab.txt] [--reps 10] [--limit 300]

Sizes: 10 000 points against 8, 20 and 50 surfaces (planes 120 x 120, spheres 100 x 100, cylinders 200 x 60, open and
closed splines 30 x 30 / 31 x 30: the grids of surface._TRIM, trimmed by the occupancy kernel with the default
thresholds around the shape's own points), and a batch of 4 shapes of 20.  The parent starts one child process per
size under its own time limit and stops at the first that fails; a child warms both variants up and then alternates
them, timing the distance launch with the library's HIP events (PN_PROF) and the whole call with torch events."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(8, 1), (20, 1), (50, 1), (20, 4)]
N_POINTS = 10000


def make_shape(n_surfaces, seed):
    """(points (10 000,3) fp32, [TrimmedSurface]): every surface a patch of a randomly placed primitive's grid, the
    points spread over the patches with 0.002 noise."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from parsenet_codebase_amd import surface
    from parsenet_codebase_amd.fitting import up_sample_points_torch_memory_efficient
    rng = np.random.RandomState(seed)
    np.random.seed(seed)
    per = N_POINTS // n_surfaces
    points, surfaces = [], []
    for s in range(n_surfaces):
        n = per if s + 1 < n_surfaces else N_POINTS - per * (n_surfaces - 1)
        kind = (1, 5, 4, 2, 0)[s % 5]
        centre = rng.uniform(-0.3, 0.3, 3)
        if kind == 1:
            normal = rng.standard_normal(3)
            normal /= np.linalg.norm(normal)
            grid = surface.sample_plane(float(normal @ centre), normal, centre.reshape(1, 3))
            size = (120, 120)
        elif kind == 5:
            grid, size = surface.sample_sphere(rng.uniform(0.1, 0.25), centre), (100, 100)
        elif kind == 4:
            axis = rng.standard_normal(3)
            axis /= np.linalg.norm(axis)
            ends = centre[None] + np.outer([-0.2, 0.2], axis)
            grid, size = surface.sample_cylinder_trim(rng.uniform(0.05, 0.15), centre, axis, ends), (200, 60)
        else:
            size = (30, 30) if kind == 2 else (31, 30)
            u, v = np.meshgrid(np.linspace(-0.2, 0.2, size[0]), np.linspace(-0.2, 0.2, size[1]), indexing="ij")
            w = 0.05 * np.sin(rng.uniform(4, 9) * u) * np.cos(rng.uniform(4, 9) * v)
            frame = np.linalg.qr(rng.standard_normal((3, 3)))[0]
            grid = np.stack([u, v, w], 2).reshape(-1, 3) @ frame.T + centre
        grid = np.asarray(grid, np.float64).reshape(size[0], size[1], 3)
        # the segment's points: a window of 40 % of the grid in both directions, bilinear positions inside its cells
        wu, wv = max(2, int(0.4 * (size[0] - 1))), max(2, int(0.4 * (size[1] - 1)))
        i0, j0 = rng.randint(0, size[0] - wu), rng.randint(0, size[1] - wv)
        i, j = i0 + rng.randint(0, wu, n), j0 + rng.randint(0, wv, n)
        a, b = rng.uniform(size=(n, 1)), rng.uniform(size=(n, 1))
        p = ((1 - a) * (1 - b) * grid[i, j] + a * (1 - b) * grid[i + 1, j] + (1 - a) * b * grid[i, j + 1]
             + a * b * grid[i + 1, j + 1]) + rng.normal(0, 0.002, (n, 3))
        p = p.astype(np.float32)
        rounds, eps, _ = surface._TRIM[kind]
        cloud = up_sample_points_torch_memory_efficient(torch.from_numpy(p).cuda(), rounds)
        surfaces.append(surface.bit_mapping_points_torch(cloud, grid.reshape(-1, 3), eps, size[0], size[1]))
        points.append(p)
    return np.concatenate(points), surfaces


def child(n_surfaces, batch, reps):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from parsenet_codebase_amd import _lib, metrics, surface
    shapes = [make_shape(n_surfaces, 100 * n_surfaces + b) for b in range(batch)]
    pts = [torch.from_numpy(p).cuda() for p, _ in shapes]
    surfs = [s for _, s in shapes]
    faces = [sum(2 * int(m.mask.sum()) for m in s) for s in surfs]
    area_cells = [sum(m.mask.size for m in s) for s in surfs]

    def run(prune):
        _lib.prof_reset()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = surface.point_surface_distance(pts, surfs, prune=prune, return_index=True)
        t1.record()
        torch.cuda.synchronize()
        prof = _lib.prof_results()
        return out, prof["trimesh_point_dist"][0], prof["trimesh_records"][0], t0.elapsed_time(t1)

    _lib.prof_enable(True)
    ref = None
    for prune in (True, False, True, False):                    # warm-up, both variants twice
        out = run(prune)[0]
        ref = ref or out
        assert all(torch.equal(x, y) for a, b in zip(ref, out) for x, y in zip(a, b)), "pruning changed a result"
    times = {True: [], False: []}
    for _ in range(reps):
        for prune in (True, False):
            times[prune].append(run(prune)[1:])
    _lib.prof_enable(False)
    run(True)
    skipped, visits = int(surface.LAST_PRUNE["skipped"].item()), surface.LAST_PRUNE["visits"]
    print("%d surfaces x batch %d: %s kept triangles of %s cells per shape, %d points per shape"
          % (n_surfaces, batch, faces, area_cells, N_POINTS))
    for prune in (True, False):
        t = np.asarray(times[prune])
        print("  prune %-5s distance launch median %.3f ms (min %.3f, max %.3f), record launch %.3f ms, whole call "
              "%.3f ms, %d runs" % (prune, np.median(t[:, 0]), t[:, 0].min(), t[:, 0].max(), np.median(t[:, 1]),
                                    np.median(t[:, 2]), reps))
    print("  groups skipped %d of %d visits (%.1f %%); results bit-identical with pruning on and off"
          % (skipped, visits, 100.0 * skipped / visits))
    # the bias of the sampled figure: 10 000 samples per shape (numpy seed 1) against the surfaces themselves
    exact = metrics.surface_coverage_batch(pts, surfs)
    for b in range(batch):
        np.random.seed(1)
        samples = surface.sample_from_collection_of_mesh(surfs[b], N_POINTS)
        m = metrics.coverage_metrics_batch([samples], [pts[b]])[0]
        print("  shape %d: sampled sk_1 %.4f sk %.5f (%d samples) | p_cover_surface %.4f p_dist_surface %.5f"
              % (b, m["sk_1"], m["sk"], samples.shape[0], exact[b]["p_cover_surface"], exact[b]["p_dist_surface"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tridist_ab.txt"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--limit", type=int, default=300, help="seconds per size")
    ap.add_argument("--child", nargs=2, type=int, metavar=("SURFACES", "BATCH"))
    args = ap.parse_args()
    if args.child:
        child(args.child[0], args.child[1], args.reps)
        return 0
    lines = []
    for n_surfaces, batch in SIZES:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child",
               str(n_surfaces), str(batch), "--reps", str(args.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        lines.append(r.stdout)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            print("size (%d, %d) ended with status %d: stopping" % (n_surfaces, batch, r.returncode))
            return r.returncode
    with open(args.out, "w") as f:
        f.write("tools/tridist_ab.py: MI355X, %d alternating runs per variant after two warm-up runs of each\n"
                % args.reps)
        f.write("".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
