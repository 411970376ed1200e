"""Timing of the Euclidean cluster extraction (csrc/cluster.hip) beside the host route a user has without it.

    python tools/cluster_ab.py [--out profiles/cluster.txt] [--reps 20] [--limit 300]

Sizes: 10 000, 100 000 and 1 000 000 points and a batch of 4 x 10 000.  Each cloud is a scene of five jittered tori
(R = 1, r = 0.3, four apart) that share 99 % of the points, plus five clumps of debris (cubes at the density of the
tori) that share the rest; the clouds of a batch have different seeds.  The radius is three times the mean spacing of
the points on the tori.  The parent starts one child process per size under its own time limit and stops at the first
that fails; a child makes two warm-up calls and then times ``kernels.cluster_ragged`` (every output, min_size 1) with
HIP events, median of --reps runs, and prints the launches, the rounds that did work (the control words at the head of
the workspace, read after one extra call through the C ABI), the components it found and the time per point.  Beside
it, alternating in the same run:
  host route  download, ``scipy.spatial.cKDTree.query_pairs(r)``, ``scipy.sparse.csgraph.connected_components``,
              upload of the labels; wall clock, HOST_RUNS runs spread between the timed calls.  The tree decides on fp64
              distances, so only the number of components is compared.  Where scipy does not import the route is left out
              and the line says so."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(10000, 1), (100000, 1), (1000000, 1), (10000, 4)]
TORI, CLUMPS, DEBRIS = 5, 5, 0.01
AREA = 4 * 3.141592653589793 ** 2 * 1.0 * 0.3
HOST_RUNS = 3


def scene(n, seed):
    """(n,3) fp32 and the radius: five jittered tori, five clumps of debris, shuffled."""
    import numpy as np
    rng = np.random.RandomState(seed)
    debris = max(CLUMPS, int(n * DEBRIS))
    per = (n - debris) // TORI
    parts = []
    for t in range(TORI):
        m = per if t else n - debris - per * (TORI - 1)
        u, v = rng.uniform(0, 2 * np.pi, (2, m))
        P = np.stack([(1 + 0.3 * np.cos(v)) * np.cos(u), (1 + 0.3 * np.cos(v)) * np.sin(u), 0.3 * np.sin(v)], 1)
        spacing = (AREA / m) ** 0.5
        parts.append(P + 0.1 * spacing * rng.normal(size=P.shape) + np.asarray([4.0 * t, 0.0, 0.0]))
    for c in range(CLUMPS):
        m = debris // CLUMPS + (1 if c < debris % CLUMPS else 0)
        parts.append(spacing * m ** (1 / 3) * rng.uniform(-0.5, 0.5, (m, 3)) + np.asarray([4.0 * c + 2.0, 2.5, 0.0]))
    P = np.concatenate(parts).astype(np.float32)
    return P[rng.permutation(n)], float(np.float32(3 * (AREA / per) ** 0.5))


def host_route(torch, pts, r):
    """One cloud on the GPU -> (labels on the GPU, components), by scipy on the host."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree
    import numpy as np
    P = pts.cpu().numpy()
    pairs = cKDTree(P).query_pairs(r, output_type="ndarray")
    n = P.shape[0]
    graph = coo_matrix((np.ones(len(pairs), np.int8), (pairs[:, 0], pairs[:, 1])), shape=(n, n))
    C, label = connected_components(graph, directed=False)
    out = torch.from_numpy(label.astype(np.int32)).to(pts.device)
    torch.cuda.synchronize()
    return out, C


def _timed(torch, fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    out = fn()
    t1.record()
    torch.cuda.synchronize()
    return out, t0.elapsed_time(t1)


def rounds_worked(torch, lib, flat, off, rad, max_n):
    """One call through the C ABI on a workspace of our own -> the rounds in which a component found an edge."""
    from parsenet_codebase_amd._lib import check, current_stream, ptr
    total, S = flat.shape[0], rad.shape[0]
    wsz = lib.pn_cluster_workspace_bytes(total, S)
    ws = torch.empty(wsz, dtype=torch.uint8, device=flat.device)
    assert ws.data_ptr() % 16 == 0
    label = torch.empty(total, dtype=torch.int32, device=flat.device)
    ncomp = torch.empty(S, dtype=torch.int32, device=flat.device)
    check(lib.pn_cluster_f32(ptr(flat), ptr(off), S, total, max_n, ptr(rad), 1, ptr(label), ptr(ncomp), None, None, None,
                             ptr(ws), wsz, current_stream(flat.device)), "pn_cluster_f32")
    torch.cuda.synchronize()
    return int(ws[:4 * 32].view(torch.int32).sum())


def child(n, batch, reps):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from parsenet_codebase_amd import _lib, kernels
    lib = _lib.load()
    clouds = [scene(n, 4 + b) for b in range(batch)]
    pts = torch.from_numpy(np.stack([c[0] for c in clouds])).cuda()
    flat = pts.reshape(-1, 3)
    off = torch.arange(batch + 1, dtype=torch.int32, device=pts.device) * n
    rad = torch.tensor([c[1] for c in clouds], dtype=torch.float32, device=pts.device)
    try:
        import scipy  # noqa: F401
        have_scipy = True
    except ImportError:
        have_scipy = False

    def ours():
        return kernels.cluster_ragged(flat, off, rad, 1)

    def theirs():
        return [host_route(torch, pts[b], clouds[b][1]) for b in range(batch)]

    ref = _timed(torch, ours)[0]
    assert all(torch.equal(a, b) for a, b in zip(ref, _timed(torch, ours)[0])), "a second run changed a result"
    t, th = [], []
    host_at = set(int(v) for v in np.linspace(0, reps - 1, HOST_RUNS)) if have_scipy else set()
    for rep in range(reps):                                      # the competitors alternate in one run
        t.append(_timed(torch, ours)[1])
        if rep in host_at:
            w0 = time.perf_counter()
            other = theirs()
            th.append(1e3 * (time.perf_counter() - w0))
    t = np.asarray(t)
    ncomp = ref[1].tolist()
    worked = rounds_worked(torch, lib, flat, off, rad, batch * n)
    launches = lib.pn_cluster_launches(batch * n)
    line = ("%d x %d points, radius %.5f -> %s components (largest %d, %d of %d points in components below 50): %d "
            "launches scheduled, %d rounds did work, workspace %.1f MB, median %.3f ms (min %.3f, max %.3f), %.2f ns per "
            "point; %d runs"
            % (batch, n, clouds[0][1], " + ".join(str(v) for v in ncomp), int(ref[2].max()),
               int(ref[2][(ref[2] > 0) & (ref[2] < 50)].sum()), batch * n, launches, worked,
               lib.pn_cluster_workspace_bytes(batch * n, batch) / 1e6, np.median(t), t.min(), t.max(),
               1e6 * np.median(t) / (batch * n), reps))
    if have_scipy:
        th = np.asarray(th)
        found = [o[1] for o in other]
        line += ("; host route (download, cKDTree.query_pairs, connected_components, upload), wall clock, same run, %d "
                 "runs: median %.1f ms (min %.1f, max %.1f): %.1f times the kernels' time"
                 % (len(th), np.median(th), th.min(), th.max(), np.median(th) / np.median(t)))
        line += "; the same components" if found == ncomp else "; it found %r components (fp64 distances)" % (found,)
    else:
        line += "; host route left out: scipy does not import here"
    print(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--limit", type=int, default=300, help="seconds per size")
    ap.add_argument("--child", nargs=2, type=int, metavar=("N", "BATCH"))
    args = ap.parse_args()
    if args.child:
        child(args.child[0], args.child[1], args.reps)
        return 0
    lines = []
    for n, batch in SIZES:
        job = ["--child", str(n), str(batch)]
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__)] + job + [
            "--reps", str(args.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        lines.append(r.stdout)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            print("%s ended with status %d: stopping" % (" ".join(job), r.returncode))
            return r.returncode
    with open(args.out, "w") as f:
        f.write("tools/cluster_ab.py: MI355X, %d timed runs per size after two warm-up runs, HIP events; label, ncomp, "
                "count, first and ndrop, min_size 1\n" % args.reps)
        f.write("".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
