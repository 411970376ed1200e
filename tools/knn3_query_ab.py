"""Timing of the cross-cloud neighbour query (csrc/knn3_query.hip) and of k-NN lifting on it, beside the brute-force
Chamfer kernel and with / without the binning of the queries into the reference's cells.

    python tools/knn3_query_ab.py [--out profiles/knn3_query.txt] [--reps 20] [--limit 170]

Sizes (queries x reference): 10^4 x 10^4, 10^5 x 10^4, 10^6 x 10^4, 10^6 x 10^5, 10^6 x 10^6 and a batch of
4 x (10^4 x 10^4).  Both clouds are jittered tori (tools/orient_normals_ab.py) with different seeds, their rows
shuffled (a second scan does not arrive in the cell order of the first).  Queries "on the surface": the second torus as
it is; "far": the same torus moved by (2, 2, 2), outside the reference's box.  k = 1 and k = 3.
The parent starts one child process per size under its own time limit and stops at the first that fails.  A child
times with HIP events: two warm-up calls, then the median of --reps calls; a measurement whose first call takes more
than 100 ms is repeated 3 times, one above 1 s not at all (the line says so).  In the same process, alternating:
  query        ``kernels.knn3_query`` with distances, queries binned (the default) and PN_KNN3_QUERY_BIN=0
  lift         ``neighbors.lift_knn`` of 8 fp32 channels per sample (query + interpolation), binned and not
  chamfer      ``kernels.chamfer_nn_ragged`` one-sided, for k = 1, while a call is predicted (from the pairs per
               second of the size before) to stay under 3 s; the sizes it is not run at are named."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(10 ** 4, 10 ** 4, 1), (10 ** 5, 10 ** 4, 1), (10 ** 6, 10 ** 4, 1), (10 ** 6, 10 ** 5, 1),
         (10 ** 6, 10 ** 6, 1), (10 ** 4, 10 ** 4, 4)]
CHANNELS = 8
CHAMFER_PAIRS_PER_S = 2.0e11       # a cautious first guess; every measured size replaces it


def cloud(n, seed):
    import numpy as np
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from orient_normals_ab import jittered_torus
    P = jittered_torus(n, seed=seed)[0]
    return P[np.random.RandomState(seed).permutation(n)].copy()


def child(nq, nr, batch, reps, rate):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from parsenet_codebase_amd import kernels, neighbors
    from parsenet_codebase_amd.ragged import Clouds
    ref = torch.from_numpy(np.stack([cloud(nr, 4 + b) for b in range(batch)])).cuda()
    surface = torch.from_numpy(np.stack([cloud(nq, 40 + b) for b in range(batch)])).cuda()
    values = torch.randn(batch, nr, CHANNELS, generator=torch.Generator().manual_seed(0)).cuda()
    rc = Clouds(ref, "knn3_query_ab")

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = fn()
        t1.record()
        torch.cuda.synchronize()
        return out, t0.elapsed_time(t1)

    def measure(fn):
        """-> (result, median ms, runs): two warm-ups, then 20 / 3 / 0 timed calls by the cost of the first."""
        out, first = timed(fn)
        if first > 1000.0:
            return out, first, 0
        timed(fn)
        n = reps if first <= 100.0 else min(reps, 3)
        return out, float(np.median([timed(fn)[1] for _ in range(n)])), n

    def binned(on, fn):
        os.environ["PN_KNN3_QUERY_BIN"] = "1" if on else "0"
        try:
            return measure(fn)
        finally:
            os.environ.pop("PN_KNN3_QUERY_BIN", None)

    fmt = lambda m: "%.3f ms (%d runs)" % (m[1], m[2]) if m[2] else "%.0f ms (one call, not repeated)" % m[1]  # noqa: E731
    for where, qry in (("surface", surface), ("far", surface + 2.0)):
        qc = Clouds(qry, "knn3_query_ab")
        for k in (1, 3):
            q1 = binned(True, lambda: kernels.knn3_query(rc.flat, rc, qc.flat, qc, k, want_dist=True))
            q0 = binned(False, lambda: kernels.knn3_query(rc.flat, rc, qc.flat, qc, k, want_dist=True))
            assert torch.equal(q1[0][0], q0[0][0]) and torch.equal(q1[0][1], q0[0][1]), "the binning moved a result"
            l1 = binned(True, lambda: neighbors.lift_knn(values, qry, ref, k=k))
            l0 = binned(False, lambda: neighbors.lift_knn(values, qry, ref, k=k))
            line = ("%d x (%d queries x %d reference), %s, k = %d: query binned %s, not binned %s; lift_knn (%d channels) "
                    "binned %s, not binned %s" % (batch, nq, nr, where, k, fmt(q1), fmt(q0), CHANNELS, fmt(l1), fmt(l0)))
            if k == 1:
                pairs = float(batch) * nq * nr
                if pairs / rate > 3.0:
                    line += "; chamfer_nn_ragged NOT RUN (predicted %.0f s per call)" % (pairs / rate)
                else:
                    c = measure(lambda: kernels.chamfer_nn_ragged(qc.flat, qc.device_offsets(), nq, rc.flat,
                                                                  rc.device_offsets(), nr, side_b=False))
                    same = torch.equal(c[0][1], q1[0][0][:, 0].long())
                    rate = pairs / (c[1] * 1e-3)
                    line += "; chamfer_nn_ragged one-sided %s, %s neighbours" % (fmt(c), "the same" if same else "OTHER")
            print(line)
            sys.stdout.flush()
    print("rate %g" % rate)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn3_query.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--limit", type=int, default=170, help="seconds per size")
    ap.add_argument("--child", nargs=3, type=int, metavar=("NQ", "NR", "BATCH"))
    ap.add_argument("--rate", type=float, default=CHAMFER_PAIRS_PER_S)
    args = ap.parse_args()
    if args.child:
        child(args.child[0], args.child[1], args.child[2], args.reps, args.rate)
        return 0
    lines, rate = [], args.rate
    for nq, nr, batch in SIZES:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", str(nq),
               str(nr), str(batch), "--reps", str(args.reps), "--rate", repr(rate)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        body = [l for l in r.stdout.splitlines(True) if not l.startswith("rate ")]
        rate = ([rate] + [float(l.split()[1]) for l in r.stdout.splitlines() if l.startswith("rate ")])[-1]
        sys.stdout.write("".join(body))
        sys.stdout.flush()
        lines += body
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            print("size (%d x %d, batch %d) ended with status %d: stopping" % (nq, nr, batch, r.returncode))
            return r.returncode
    with open(args.out, "w") as f:
        f.write("tools/knn3_query_ab.py: MI355X, HIP events, median of %d timed calls after two warm-up calls (3 where a "
                "call takes more than 100 ms); jittered tori, rows shuffled; far = queries moved by (2, 2, 2)\n"
                % args.reps)
        f.write("".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
