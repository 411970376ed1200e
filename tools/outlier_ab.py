"""Timing of the statistical outlier removal (csrc/outlier.hip) beside the same definition written as tensor expressions.

    python tools/outlier_ab.py [--out profiles/outlier.txt] [--reps 20] [--limit 300]

Sizes: 10 000, 100 000 and 1 000 000 points and a batch of 4 x 10 000, each cloud a jittered torus
(tools/orient_normals_ab.py) with 0.2 % of its points replaced by strays 2 .. 4 from the origin, the clouds of a batch
with different seeds; k = 20, std_ratio = 2.  The parent starts one child process per size under its own time limit and
stops at the first that fails; a child makes two warm-up calls and then times, with HIP events, median of --reps runs,
  statistic   ``kernels.outlier_stat`` alone (six launches) on the distances of one ``knn3_grid`` search,
  whole call  ``cleaning.outlier_statistic(search="grid")``: the search and the statistic,
  torch       the same definition on the same distances as tensor expressions: the fp64 mean over k, masked sums per
              cloud, the comparison and ``torch.nonzero`` (which synchronises).  Its sums are torch's, not the fixed
              tree, so a mask may differ where a statistic lies within rounding of the threshold: the number of
              differing points is a figure, not an assertion."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(10000, 1), (100000, 1), (1000000, 1), (10000, 4)]
K, RATIO = 20, 2.0


def scan(n, seed):
    import numpy as np
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from orient_normals_ab import jittered_torus
    rng = np.random.RandomState(seed)
    P = jittered_torus(n, seed=seed)[0].copy()
    m = n // 500
    v = rng.normal(size=(m, 3))
    P[rng.permutation(n)[:m]] = (v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(2, 4, (m, 1))).astype(np.float32)
    return P


def torch_statistic(dist, batch, n, ratio):
    """(keep (batch,n), index): the definition as tensor expressions on dist (batch*n, k)."""
    import torch
    a = dist.double().mean(1).reshape(batch, n)
    valid = a > 0
    mean = torch.where(valid, a, torch.zeros_like(a)).sum(1, keepdim=True) / n
    std = (torch.where(valid, (a - mean) ** 2, torch.zeros_like(a)).sum(1, keepdim=True) / (n - 1)).sqrt()
    keep = valid & (a < mean + ratio * std)
    return keep, torch.nonzero(keep)


def child(n, batch, reps):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from parsenet_codebase_amd import _lib, cleaning, kernels
    from parsenet_codebase_amd.ragged import Clouds
    lib = _lib.load()
    pts = torch.from_numpy(np.stack([scan(n, 4 + b) for b in range(batch)])).cuda()
    clouds = Clouds(pts, "outlier_ab")
    dist = kernels.knn3_grid(clouds.flat, clouds, None, K, want_dist=True)[1]

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = fn()
        t1.record()
        torch.cuda.synchronize()
        return out, t0.elapsed_time(t1)

    def measure(fn):
        ref = timed(fn)[0]
        timed(fn)                                                                             # two warm-ups
        return ref, np.asarray([timed(fn)[1] for _ in range(reps)])

    ours, t = measure(lambda: kernels.outlier_stat(dist, clouds, K, RATIO))
    assert all(torch.equal(a, b) for a, b in zip(ours, kernels.outlier_stat(dist, clouds, K, RATIO))), "a second run changed a result"
    _, tw = measure(lambda: cleaning.outlier_statistic(pts, K, RATIO, search="grid"))
    other, tt = measure(lambda: torch_statistic(dist, batch, n, RATIO))
    differ = int((other[0].reshape(-1) != ours[2]).sum())
    kept = ours[3].tolist()
    gbs = (4.0 * K + 8 + 8 + 8 + 1 + 1 + 4) * batch * n / (np.median(t) * 1e-3) / 1e9
    print("%d x %d points, k = %d, std_ratio = %g: kept %s; statistic alone %d launches, median %.3f ms (min %.3f, max "
          "%.3f), %.0f GB/s of the %d bytes per point it reads and writes; whole call (grid search + statistic) median "
          "%.3f ms (min %.3f); torch expressions on the same distances median %.3f ms (min %.3f), %d points differ; "
          "%d runs" % (batch, n, K, RATIO, kept, lib.pn_outlier_launches(), np.median(t), t.min(), t.max(), gbs,
                       4 * K + 30, np.median(tw), tw.min(), np.median(tt), tt.min(), differ, reps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "outlier.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--limit", type=int, default=300, help="seconds per size")
    ap.add_argument("--child", nargs=2, type=int, metavar=("N", "BATCH"))
    args = ap.parse_args()
    if args.child:
        child(args.child[0], args.child[1], args.reps)
        return 0
    lines = []
    for n, batch in SIZES:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", str(n),
               str(batch), "--reps", str(args.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        lines.append(r.stdout)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            print("size (%d points, batch %d) ended with status %d: stopping" % (n, batch, r.returncode))
            return r.returncode
    with open(args.out, "w") as f:
        f.write("tools/outlier_ab.py: MI355X, %d timed runs per size after two warm-up runs, HIP events; jittered torus "
                "with 0.2 %% strays\n" % args.reps)
        f.write("".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
