"""Timing of the consistent normal orientation (csrc/orient.hip) beside the only alternative there was before it.

    python tools/orient_normals_ab.py [--out profiles/orient_normals.txt] [--reps 20] [--limit 180]

Sizes: one cloud of 10 000 points at k = 8, 16 and 32, and a batch of 4 such clouds at k = 16.  The clouds are
synthetic.make_batch shapes (patches of analytic primitives), their normals estimate_normals' canonical-sign ones.
The parent starts one child process per size under its own time limit and stops at the first that fails; a child
makes two warm-up calls and then times the orientation launch and the neighbour search with the library's HIP events
(PN_PROF) and the whole orient_normals call with torch events.  Beside it, the host path: download the normals and the
neighbour indices, scipy.sparse.csgraph.minimum_spanning_tree + breadth_first_order per cloud from the topmost point
of every connected component, upload the signs (wall clock, synchronised at both ends, the neighbour search not
included).  It also prints how many normals the two orient differently: the tie rules differ (scipy's order among
equal weights is its own, and a zero weight is no edge to it, so the weights get 1e-12 added), so that is a figure, not
an assertion.

    python tools/orient_normals_ab.py --engine global [--out ...]

times the global-memory engine (csrc/orient_global.hip) at k = 16 and rewrites its own section at the end of the file:
one synthetic.make_batch cloud of 10 000 points and a batch of 4, each beside the one-workgroup kernel on the same
input and alternating with it, and one jittered torus of 100 000 and of 1 000 000 points (a surface), where only the
global engine runs.  Median of --reps runs after two warm-up calls: the engine's launches with the library's HIP
events, the whole orient_normals call (neighbour search included) with torch events.  At 100 000 points also the host
path, wall clock, 3 runs."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(8, 1), (16, 1), (32, 1), (16, 4)]
N_POINTS = 10000
GLOBAL_SIZES = [(10000, 1), (10000, 4), (100000, 1), (1000000, 1)]
GLOBAL_K = 16
GLOBAL_MARK = "tools/orient_normals_ab.py --engine global:"


def host_orient(pts, nrm, idx):
    """One cloud on the host, numpy in and out: the signs (+1 / -1) by scipy's spanning tree of the same graph."""
    import numpy as np
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import breadth_first_order, connected_components, minimum_spanning_tree
    n, k = idx.shape
    rows = np.repeat(np.arange(n), k)
    cols = idx.reshape(-1).astype(np.int64)
    keep = rows != cols
    rows, cols = rows[keep], cols[keep]
    n64 = nrm.astype(np.float64)
    dot = (n64[rows] * n64[cols]).sum(1)
    graph = coo_matrix((np.maximum(1.0 - np.abs(dot), 0.0) + 1e-12, (rows, cols)), shape=(n, n)).tocsr()
    graph = graph.maximum(graph.T)
    tree = minimum_spanning_tree(graph)
    tree = tree.maximum(tree.T).tocsr()
    ncomp, label = connected_components(tree, directed=False)
    sign = np.zeros(n)
    for c in range(ncomp):
        members = np.flatnonzero(label == c)
        seed = int(members[np.argmax(pts[members, 2])])
        order, pred = breadth_first_order(tree, seed, directed=False)
        sign[seed] = -1.0 if nrm[seed, 2] < 0 else 1.0
        for v in order[1:]:
            p = pred[v]
            sign[v] = sign[p] * (-1.0 if (n64[v] * n64[p]).sum() < 0 else 1.0)
    return sign


def child(k, batch, reps):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from parsenet_codebase_amd import _lib, kernels, synthetic
    from parsenet_codebase_amd.point_normals import estimate_normals, orient_normals
    pts = torch.from_numpy(synthetic.make_batch(0, batch, N_POINTS)[0]).cuda()
    nrm = estimate_normals(pts, k=k)

    def run():
        _lib.prof_reset()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = orient_normals(pts, nrm, k=k, return_flags=True)
        t1.record()
        torch.cuda.synchronize()
        prof = _lib.prof_results()
        return out, prof["orient_normals"][0], prof["knn3_ragged"][0], t0.elapsed_time(t1)

    def host():
        off = torch.arange(batch + 1, dtype=torch.int32, device=pts.device) * N_POINTS
        idx = kernels.knn3_ragged(pts.reshape(-1, 3), off, N_POINTS, k).reshape(batch, N_POINTS, k)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        p, n, i = pts.cpu().numpy(), nrm.cpu().numpy(), idx.cpu().numpy()
        sign = np.stack([host_orient(p[b], n[b], i[b]) for b in range(batch)])
        out = nrm * torch.from_numpy(sign.astype(np.float32)).to(pts.device)[..., None]
        torch.cuda.synchronize()
        return out, 1e3 * (time.perf_counter() - t0)

    _lib.prof_enable(True)
    ref = run()[0]
    assert all(torch.equal(a, b) for a, b in zip(ref, run()[0])), "a second run changed a result"     # two warm-up calls
    t = np.asarray([run()[1:] for _ in range(reps)])
    _lib.prof_enable(False)
    host()
    hosted = [host() for _ in range(3)]
    differ = int((hosted[0][0] != ref[0]).any(-1).sum())
    seeds = sum(int(torch.unique(s).numel()) for s in ref[2])
    print("%d x %d points, k = %d: orientation launch median %.3f ms (min %.3f, max %.3f), neighbour search %.3f ms, "
          "whole call %.3f ms, %d runs; host path (download, scipy spanning tree and walk, upload) median %.1f ms of 3; "
          "%d connected component(s); %d of %d normals oriented differently by the host path"
          % (batch, N_POINTS, k, np.median(t[:, 0]), t[:, 0].min(), t[:, 0].max(), np.median(t[:, 1]),
             np.median(t[:, 2]), reps, np.median([h[1] for h in hosted]), seeds, differ, batch * N_POINTS))


def jittered_torus(n, R=0.7, r=0.25, seed=4):
    """n points of a jittered nu x nv grid on the torus around the z axis (the tests' torus at any size): nv the
    largest divisor of n up to sqrt(n / 2), so that nu is about 2 nv."""
    import numpy as np
    nv = max(d for d in range(1, int((n / 2.0) ** 0.5) + 1) if n % d == 0)
    nu = n // nv
    rng = np.random.RandomState(seed)
    u, v = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    u = 2 * np.pi * (u + 0.25 * rng.uniform(-1, 1, u.shape)).reshape(-1) / nu
    v = 2 * np.pi * (v + 0.25 * rng.uniform(-1, 1, v.shape)).reshape(-1) / nv
    out = np.stack([np.cos(v) * np.cos(u), np.cos(v) * np.sin(u), np.sin(v)], 1)
    pts = np.stack([R * np.cos(u), R * np.sin(u), np.zeros_like(u)], 1) + r * out
    return pts.astype(np.float32)[None]


def child_global(n, batch, reps):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from parsenet_codebase_amd import _lib, kernels, synthetic
    from parsenet_codebase_amd.point_normals import estimate_normals, orient_normals
    k = GLOBAL_K
    lib = _lib.load()
    small = n <= lib.pn_orient_normals_max_points()
    pts = torch.from_numpy(synthetic.make_batch(0, batch, n)[0] if small else jittered_torus(n)).cuda()
    n = pts.shape[1]
    nrm = estimate_normals(pts, k=k, search="auto")

    def run(engine):
        _lib.prof_reset()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = orient_normals(pts, nrm, k=k, return_flags=True, search="auto", engine=engine)
        t1.record()
        torch.cuda.synchronize()
        prof = _lib.prof_results()
        return out, prof["orient_normals_global" if engine else "orient_normals"][0], t0.elapsed_time(t1)

    engines = ("global", None) if small else ("global",)
    _lib.prof_enable(True)
    ref = {e: run(e)[0] for e in engines}
    for e in engines:                                                                       # two warm-up calls each
        assert all(torch.equal(a, b) for a, b in zip(ref["global"], run(e)[0])), "engine %r changed a result" % (e,)
    t = {e: [] for e in engines}
    for _ in range(reps):                                                                   # alternating
        for e in engines:
            t[e].append(run(e)[1:])
    _lib.prof_enable(False)
    t = {e: np.asarray(v) for e, v in t.items()}
    seeds = sum(int(torch.unique(s).numel()) for s in ref["global"][2])
    line = ("%d x %d points, k = %d: global engine, %d launches scheduled: median %.3f ms (min %.3f, max %.3f), whole "
            "call %.3f ms, %d runs"
            % (batch, n, k, lib.pn_orient_normals_global_launches(n), np.median(t["global"][:, 0]),
               t["global"][:, 0].min(), t["global"][:, 0].max(), np.median(t["global"][:, 1]), reps))
    if small:
        line += ("; one-workgroup kernel on the same input: median %.3f ms (min %.3f, max %.3f), whole call %.3f ms; "
                 "the same bits" % (np.median(t[None][:, 0]), t[None][:, 0].min(), t[None][:, 0].max(),
                                    np.median(t[None][:, 1])))
    if n == 100000:
        off = torch.tensor([0, n], dtype=torch.int32, device=pts.device)
        idx = kernels.knn3_grid(pts.reshape(-1, 3), off, n, k)
        torch.cuda.synchronize()
        walls = []
        for _ in range(3):
            t0 = time.perf_counter()
            sign = host_orient(pts[0].cpu().numpy(), nrm[0].cpu().numpy(), idx.cpu().numpy())
            out = nrm[0] * torch.from_numpy(sign.astype(np.float32)).to(pts.device)[:, None]
            torch.cuda.synchronize()
            walls.append(1e3 * (time.perf_counter() - t0))
        differ = int((out != ref["global"][0][0]).any(-1).sum())
        line += ("; host path (download, scipy spanning tree and walk, upload), wall clock: %s ms; %d of %d normals "
                 "oriented differently by it" % (", ".join("%.1f" % w for w in walls), differ, n))
    print(line + "; %d connected component(s)" % seeds)


def main_global(args):
    lines = []
    for n, batch in GLOBAL_SIZES:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child-global",
               str(n), str(batch), "--reps", str(args.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        lines.append(r.stdout)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            print("size (%d points, batch %d) ended with status %d: stopping" % (n, batch, r.returncode))
            return r.returncode
    kept = open(args.out).read() if os.path.exists(args.out) else ""
    kept = kept[:kept.index(GLOBAL_MARK)] if GLOBAL_MARK in kept else kept
    with open(args.out, "w") as f:
        f.write(kept.rstrip("\n") + "\n\n" if kept.strip() else "")
        f.write("%s MI355X, k = %d, %d timed runs per size after two warm-up runs, the engines alternating\n"
                % (GLOBAL_MARK, GLOBAL_K, args.reps))
        f.write("".join(lines))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "orient_normals.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--limit", type=int, default=180, help="seconds per size")
    ap.add_argument("--child", nargs=2, type=int, metavar=("K", "BATCH"))
    ap.add_argument("--child-global", nargs=2, type=int, metavar=("N", "BATCH"))
    ap.add_argument("--engine", choices=("global",), help="time the global-memory engine (its own section of --out)")
    args = ap.parse_args()
    if args.child_global:
        child_global(args.child_global[0], args.child_global[1], args.reps)
        return 0
    if args.engine == "global":
        return main_global(args)
    if args.child:
        child(args.child[0], args.child[1], args.reps)
        return 0
    lines = []
    for k, batch in SIZES:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", str(k),
               str(batch), "--reps", str(args.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        lines.append(r.stdout)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            print("size (k = %d, batch %d) ended with status %d: stopping" % (k, batch, r.returncode))
            return r.returncode
    kept = open(args.out).read() if os.path.exists(args.out) else ""
    kept = "\n" + kept[kept.index(GLOBAL_MARK):] if GLOBAL_MARK in kept else ""        # the global engine's section stays
    with open(args.out, "w") as f:
        f.write("tools/orient_normals_ab.py: MI355X, %d timed runs per size after two warm-up runs\n" % args.reps)
        f.write("".join(lines) + kept)
    return 0


if __name__ == "__main__":
    sys.exit(main())
