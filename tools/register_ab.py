"""Timing of the rigid registration (csrc/register.hip) beside the host route on the same inputs.

    python tools/register_ab.py [--out profiles/register.txt] [--reps 20] [--limit 240] [--iters 10]

Sizes (source x target): 10^4 x 10^4, 10^5 x 10^5, 10^6 x 10^6 and a batch of 4 x (10^4 x 10^4), in both modes.  The
target is a jittered torus (tools/orient_normals_ab.py) with shuffled rows and its analytic normals; the source is that
cloud moved by 5 degrees about (1, 2, 3) and by (0.05, -0.03, 0.04), its rows shuffled again.  The tolerances are 0, so
that every call runs exactly --iters iterations and the final evaluation.
The parent starts one child process per size under its own time limit and stops at the first that fails.  A child
times with HIP events: two warm-up calls, then the median of --reps calls; a measurement whose first call takes more
than 100 ms is repeated 3 times, one above 1 s not at all (the line says so).  Per size and mode:
  call         ``kernels.register_ragged`` with --iters iterations, and with 1: their difference / (--iters - 1) is the
               cost of one iteration, the rest the grid build, the init and the final evaluation
  phases       one further call under the library's event profiler: the share of move, search (the two memsets and the
               query's four launches), sums (both passes) and solve (means and solve) in the whole call
  host         download, ``scipy.spatial.cKDTree`` on the target, --iters times query + numpy Kabsch (SVD) + move, upload:
               wall clock, the best of 3 runs (1 at 10^6); point to point only"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(10 ** 4, 1), (10 ** 5, 1), (10 ** 6, 1), (10 ** 4, 4)]
PHASES = ("register_move", "register_search", "register_sums", "register_solve")


def scene(n, seed):
    """(source, target, normals) fp32 numpy."""
    import numpy as np
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from orient_normals_ab import jittered_torus
    rng = np.random.RandomState(seed)
    T = jittered_torus(n, seed=seed)[0][rng.permutation(n)].astype(np.float64)
    ring = T.copy()
    ring[:, 2] = 0.0
    ring *= 0.7 / np.maximum(np.linalg.norm(ring, axis=1, keepdims=True), 1e-12)
    N = T - ring
    N /= np.maximum(np.linalg.norm(N, axis=1, keepdims=True), 1e-12)
    a = np.asarray([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    K = np.asarray([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.radians(5.0)
    R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    S = (T @ R.T + np.asarray([0.05, -0.03, 0.04]))[rng.permutation(n)]
    return S.astype(np.float32), T.astype(np.float32), N.astype(np.float32)


def host_route(src, tgt, iters, dev):
    """One cloud pair: seconds of download + k-d tree ICP (point to point) + upload."""
    import time
    import numpy as np
    import torch
    from scipy.spatial import cKDTree
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    S, T = src.cpu().numpy().astype(np.float64), tgt.cpu().numpy().astype(np.float64)
    tree = cKDTree(T)
    M = np.eye(4)
    P = S
    for _ in range(iters):
        j = tree.query(P, k=1, workers=16)[1]
        Q = T[j]
        pm, qm = P.mean(0), Q.mean(0)
        U, _, Vt = np.linalg.svd((P - pm).T @ (Q - qm))
        D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
        R = Vt.T @ D @ U.T
        step = np.eye(4)
        step[:3, :3], step[:3, 3] = R, qm - R @ pm
        M = step @ M
        P = S @ M[:3, :3].T + M[:3, 3]
    torch.from_numpy(M).to(dev)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def child(n, batch, reps, iters):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from parsenet_codebase_amd import _lib, kernels
    dev = torch.device("cuda")
    parts = [scene(n, 11 + b) for b in range(batch)]
    src, tgt, nrm = (torch.from_numpy(np.concatenate([p[k] for p in parts])).to(dev) for k in range(3))
    off = torch.from_numpy((np.arange(batch + 1) * n).astype(np.int32)).to(dev)

    def call(mode, max_iter):
        return kernels.register_ragged(src, off, tgt, off, float("inf"), mode, nrm if mode else None, None, max_iter,
                                       0.0, 0.0)

    def timed(fn):
        def once():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            return t0.elapsed_time(t1)
        first = once()
        if first > 1000.0:
            return first, 1
        once()
        r = 3 if first > 100.0 else reps
        return float(np.median([once() for _ in range(r)])), r

    label = "%d x (%d x %d)" % (batch, n, n) if batch > 1 else "%d x %d" % (n, n)
    for mode, word in ((kernels.REGISTER_POINT, "point"), (kernels.REGISTER_PLANE, "plane")):
        full, r = timed(lambda: call(mode, iters))
        one, _ = timed(lambda: call(mode, 1))
        out = call(mode, iters)
        its, status = out[1].tolist(), out[2].tolist()
        _lib.prof_enable(True)
        _lib.prof_reset()
        call(mode, iters)
        torch.cuda.synchronize()
        prof = _lib.prof_results()
        _lib.prof_enable(False)
        whole = prof.get("register", (0.0, 0))[0]
        share = "  ".join("%s %4.1f %%" % (p.split("_")[1], 100.0 * prof.get(p, (0.0, 0))[0] / whole if whole else 0.0)
                          for p in PHASES)
        print("%-22s %-5s  %9.3f ms (%d iterations, median of %d)  1 iteration: %9.3f ms  per iteration %8.3f ms  |  %s"
              "  |  iterations %s status %s" % (label, word, full, iters, r, one, (full - one) / max(iters - 1, 1), share,
                                               its, status), flush=True)
    runs = 1 if n >= 10 ** 6 else 3
    best = min(sum(host_route(src[b * n:(b + 1) * n], tgt[b * n:(b + 1) * n], iters, dev) for b in range(batch))
               for _ in range(runs))
    print("%-22s host   %9.3f ms (cKDTree + Kabsch, %d iterations, download and upload, best of %d, wall clock)"
          % (label, 1e3 * best, iters, runs), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--limit", type=int, default=240, help="seconds per size")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--child", nargs=2, type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child[0], a.child[1], a.reps, a.iters)
        return 0
    lines = ["# python tools/register_ab.py: kernels.register_ragged (csrc/register.hip) on one MI355X, HIP events;",
             "# phases from the library's event profiler in a call of their own; the host route is wall clock."]
    for n, batch in SIZES:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(n), str(batch), "--reps", str(a.reps), "--iters",
               str(a.iters)]
        try:
            run = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            lines.append("%d x %d: no result within %d s; stopping" % (n, n, a.limit))
            break
        if run.returncode != 0:
            lines.append("%d x %d: exit status %d; stopping\n%s" % (n, n, run.returncode, run.stderr[-2000:]))
            break
        lines += run.stdout.strip().split("\n")
        print(run.stdout, end="", flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    else:
        print(text)
    return 0 if not lines[-1].endswith("stopping") and "stopping\n" not in lines[-1] else 1


if __name__ == "__main__":
    sys.exit(main())
