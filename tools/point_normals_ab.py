"""Timing of the k-NN PCA point normals (csrc/normals.hip) beside the neighbour search they follow.

    python tools/point_normals_ab.py [--out profiles/point_normals.txt] [--reps 20] [--limit 120]

Sizes: one cloud of 10 000 points at k = 8, 16 and 32, and a batch of 4 such clouds at k = 16.  The clouds are
synthetic.make_batch shapes (patches of analytic primitives).  The parent starts one child process per size under its
own time limit and stops at the first that fails; a child makes two warm-up calls and then times the normals launch
and the neighbour search with the library's HIP events (PN_PROF) and the whole estimate_normals call with torch
events."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(8, 1), (16, 1), (32, 1), (16, 4)]
N_POINTS = 10000


def child(k, batch, reps):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from parsenet_codebase_amd import _lib, synthetic
    from parsenet_codebase_amd.point_normals import estimate_normals
    pts = torch.from_numpy(synthetic.make_batch(0, batch, N_POINTS)[0]).cuda()
    view = torch.tensor([0.0, 0.0, 5.0], device=pts.device)

    def run():
        _lib.prof_reset()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = estimate_normals(pts, k=k, viewpoint=view, return_scalars=True)
        t1.record()
        torch.cuda.synchronize()
        prof = _lib.prof_results()
        return out, prof["point_normals"][0], prof["knn3_ragged"][0], t0.elapsed_time(t1)

    _lib.prof_enable(True)
    ref = run()[0]
    assert all(torch.equal(a, b) for a, b in zip(ref, run()[0])), "a second run changed a result"     # two warm-up calls
    t = np.asarray([run()[1:] for _ in range(reps)])
    _lib.prof_enable(False)
    defined = float((ref[2] >= 1e-3).float().mean())
    print("%d x %d points, k = %d: normals launch median %.3f ms (min %.3f, max %.3f), neighbour search %.3f ms, whole "
          "call %.3f ms, %d runs; gap >= 1e-3 at %.1f %% of the points"
          % (batch, N_POINTS, k, np.median(t[:, 0]), t[:, 0].min(), t[:, 0].max(), np.median(t[:, 1]),
             np.median(t[:, 2]), reps, 100.0 * defined))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_normals.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--limit", type=int, default=120, help="seconds per size")
    ap.add_argument("--child", nargs=2, type=int, metavar=("K", "BATCH"))
    args = ap.parse_args()
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
    with open(args.out, "w") as f:
        f.write("tools/point_normals_ab.py: MI355X, %d timed runs per size after two warm-up runs\n" % args.reps)
        f.write("".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
