"""Timing of the uniform-grid neighbour search (csrc/knn3_grid.hip) beside the brute-force kernel and beside the only
thing a user could do above its limit before.

    python tools/knn3_grid_ab.py [--out profiles/knn3_grid.txt] [--reps 20] [--limit 240]

Where both run — one cloud of 2 000, 5 000 and 10 000 points (synthetic.make_batch shapes) at k = 8, 16 and 32, and a
batch of 4 x 10 000 at k = 16 — knn3_grid against knn3_ragged, the indices compared on the way.  Above the limit — 100 000
and 1 000 000 points at k = 16, on a surface (a torus) and in a volume (uniform in the unit cube) — knn3_grid against
block-wise fp32 coordinate differences plus torch.topk (1 024 query rows at a time, 128 at 1 000 000 points, where the first
16 384 query rows are timed and the figure is scaled to all rows, which is said on the line).
The parent starts one child process per group under its own time limit and stops at the first that fails; a child
makes two warm-up calls and then takes the median of ``reps`` calls: the whole call with torch events, every phase
with the library's HIP events (PN_PROF).  Every grid figure is taken at each points-per-cell value of PPCS (the
developer hook PN_KNN3_GRID_PPC; the value moves the speed and no output); the parent ranks them by the geometric mean
over the four large clouds and writes the best and the runner-up into the file."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PPCS = [2, 4, 8, 16, 32]
SMALL = [(n, k, 1) for n in (2000, 5000, 10000) for k in (8, 16, 32)] + [(10000, 16, 4)]
LARGE = [(n, cloud) for n in (100000, 1000000) for cloud in ("surface", "volume")]
PHASES = ("bbox", "cells", "scan", "scatter", "search")


def _timed(fn, reps):
    """Median milliseconds of ``reps`` calls after two warm-up calls (torch events), and the medians of the phases."""
    import numpy as np
    import torch
    from parsenet_codebase_amd import _lib
    fn()
    fn()
    whole, phases = [], []
    for _ in range(reps):
        _lib.prof_reset()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        prof = _lib.prof_results()
        whole.append(t0.elapsed_time(t1))
        phases.append([prof.get("knn3_grid_" + p, (0.0, 0))[0] for p in PHASES])
    return float(np.median(whole)), np.median(np.asarray(phases), 0)


def _grid_lines(what, pts, off, max_n, k, reps):
    """One line per points-per-cell value; returns {ppc: ms}."""
    from parsenet_codebase_amd import kernels
    out = {}
    for ppc in PPCS:
        os.environ["PN_KNN3_GRID_PPC"] = str(ppc)
        ms, ph = _timed(lambda: kernels.knn3_grid(pts, off, max_n, k), reps)
        out[ppc] = ms
        print("  %s, %2d points per cell: knn3_grid %8.3f ms  (%s)"
              % (what, ppc, ms, ", ".join("%s %.3f" % (p, v) for p, v in zip(PHASES, ph))))
    del os.environ["PN_KNN3_GRID_PPC"]
    return out


def child_small(reps):
    import torch
    sys.path.insert(0, ROOT)
    from parsenet_codebase_amd import _lib, kernels, synthetic
    _lib.prof_enable(True)
    for n, k, batch in SMALL:
        pts = torch.from_numpy(synthetic.make_batch(0, batch, n)[0]).cuda().reshape(-1, 3)
        off = torch.arange(batch + 1, dtype=torch.int32, device=pts.device) * n
        assert torch.equal(kernels.knn3_grid(pts, off, n, k), kernels.knn3_ragged(pts, off, n, k)), (n, k, batch)
        brute, _ = _timed(lambda: kernels.knn3_ragged(pts, off, n, k), reps)
        what = "%d x %d points, k = %d" % (batch, n, k)
        print("%s: knn3_ragged %.3f ms" % (what, brute))
        for ppc, ms in _grid_lines(what, pts, off, n, k, reps).items():
            print("RECORD small %d %d %d %d %.4f %.4f" % (n, k, batch, ppc, ms, brute))


def _cloud(n, cloud):
    import numpy as np
    rng = np.random.RandomState(n % 1000 + len(cloud))
    if cloud == "volume":
        return rng.uniform(0, 1, (n, 3)).astype(np.float32)
    u, v = rng.uniform(0, 2 * np.pi, n), rng.uniform(0, 2 * np.pi, n)       # a torus, radii 1 and 0.35
    r = 1.0 + 0.35 * np.cos(v)
    return np.stack([r * np.cos(u), r * np.sin(u), 0.35 * np.sin(v)], 1).astype(np.float32)


def _topk_fallback(pts, k, rows):
    """Block-wise fp32 differences + torch.topk over the first ``rows`` query rows."""
    import torch
    block = min(1024, max(64, (1 << 27) // pts.shape[0]))      # the (block, n, 3) differences stay near 1.5 GB
    out = []
    for a in range(0, rows, block):
        d = pts[a:min(a + block, rows), None, :] - pts[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        out.append(torch.topk(d2, k, dim=1, largest=False).indices)
    return torch.cat(out)


def child_large(n, cloud, reps):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from parsenet_codebase_amd import _lib
    _lib.prof_enable(True)
    k = 16
    pts = torch.from_numpy(_cloud(n, cloud)).cuda()
    off = torch.tensor([0, n], dtype=torch.int32, device=pts.device)
    what = "%d points (%s), k = %d" % (n, cloud, k)
    rows = n if n <= 100000 else 16384
    _topk_fallback(pts, k, rows)
    t = []
    for _ in range(3):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        _topk_fallback(pts, k, rows)
        t1.record()
        torch.cuda.synchronize()
        t.append(t0.elapsed_time(t1) * n / rows)
    fallback = float(np.median(t))
    print("%s: block-wise differences + topk %.1f ms (median of 3%s)"
          % (what, fallback, "" if rows == n else "; %d query rows timed, scaled to all rows" % rows))
    for ppc, ms in _grid_lines(what, pts, off, n, k, reps).items():
        print("RECORD large %d %s %d %d %.4f %.4f" % (n, cloud, k, ppc, ms, fallback))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn3_grid.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--limit", type=int, default=240, help="seconds per group")
    ap.add_argument("--child", nargs="+", metavar="GROUP")
    args = ap.parse_args()
    if args.child:
        if args.child[0] == "small":
            child_small(args.reps)
        else:
            child_large(int(args.child[1]), args.child[2], args.reps)
        return 0
    lines, records = [], []
    for group in [["small"]] + [["large", str(n), cloud] for n, cloud in LARGE]:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--reps",
               str(args.reps), "--child"] + group
        r = subprocess.run(cmd, capture_output=True, text=True)
        shown = "".join(l + "\n" for l in r.stdout.splitlines() if not l.startswith("RECORD"))
        records += [l.split() for l in r.stdout.splitlines() if l.startswith("RECORD")]
        sys.stdout.write(shown)
        sys.stdout.flush()
        lines.append(shown)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            print("group %s ended with status %d: stopping" % (" ".join(group), r.returncode))
            return r.returncode
    import math
    large = [r for r in records if r[1] == "large"]
    score = {ppc: math.exp(sum(math.log(float(r[6])) for r in large if int(r[5]) == ppc) / len(LARGE)) for ppc in PPCS}
    rank = sorted(PPCS, key=lambda p: score[p])
    summary = ["points per cell, geometric mean over the %d large clouds: %s\n"
               % (len(LARGE), ", ".join("%d: %.3f ms" % (p, score[p]) for p in PPCS)),
               "chosen: %d points per cell (KG_PPC of csrc/knn3_grid_math.h); runner-up: %d\n" % (rank[0], rank[1])]
    sys.stdout.write("".join(summary))
    with open(args.out, "w") as f:
        f.write("tools/knn3_grid_ab.py: MI355X, median of %d timed calls per figure after two warm-up calls\n" % args.reps)
        f.write("".join(lines + summary))
    return 0


if __name__ == "__main__":
    sys.exit(main())
