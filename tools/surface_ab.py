"""A/B of the grid-occupancy step of the trimmed surfaces (surface.grid_occupancy) at the workload's size: (a) the
ragged Chamfer kernel — nearest cloud point per cell centre, then the comparison — against (b) the dedicated
threshold kernel of csrc/surface.hip.  Same process, same inputs, alternating, HIP events.

    python tools/surface_ab.py --out profiles/surface_occupancy_ab.txt

A synthetic shape of 20 segments of 200-2 000 points with the grids of surface.trimmed_surfaces (plane 120 x 120,
cylinder 200 x 60, sphere 100 x 100, cone 99 x 51, open spline 30 x 30, closed spline 31 x 30), the clouds up-sampled
x8 / x4 like there (rows appended with small noise: the sizes are what matters), at the per-type default thresholds
and at test.py's epsilon = 0.1.  Per case: warm-up, then --repeats timed repetitions of each path, median
[min .. max] in ms, and whether the masks are identical."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from parsenet_codebase_amd import surface  # noqa: E402

KINDS = [("plane", (120, 120), 8, 0.02), ("cylinder", (200, 60), 8, 0.03), ("sphere", (100, 100), 4, 0.03),
         ("cone", (99, 51), 8, 0.03), ("open", (30, 30), 4, 0.06), ("closed", (31, 30), 4, 0.06)]


def make_shape(rng, segments, dev):
    grids, sizes, clouds, thres = [], [], [], []
    for s in range(segments):
        _, (su, sv), up, th = KINDS[s % len(KINDS)]
        u, v = np.meshgrid(np.linspace(-0.5, 0.5, su), np.linspace(-0.5, 0.5, sv), indexing="ij")
        a, b = rng.uniform(-0.5, 0.5, 2)
        g = np.stack([u, v, a * u * u + b * v * v], 2).reshape(-1, 3) + rng.uniform(-0.3, 0.3, 3)
        n = int(rng.randint(200, 2001))
        # the segment covers a part of its fitted surface, like a trimmed patch does
        part = g[(g[:, 0] - g[:, 0].mean() < rng.uniform(-0.2, 0.4))]
        base = part[rng.randint(0, part.shape[0], n)] + 0.005 * rng.randn(n, 3)
        cloud = np.concatenate([base] + [base + 0.004 * rng.randn(n, 3) for _ in range(up - 1)])
        grids.append(torch.from_numpy(g.astype(np.float32)).to(dev))
        sizes.append((su, sv))
        clouds.append(torch.from_numpy(cloud.astype(np.float32)).to(dev))
        thres.append(th)
    return grids, sizes, clouds, thres


def stats(v):
    v = sorted(v)
    return "%8.3f [%8.3f .. %8.3f]" % (v[len(v) // 2], v[0], v[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--segments", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    grids, sizes, clouds, thres = make_shape(np.random.RandomState(11), a.segments, dev)
    cells = sum((u - 1) * (v - 1) for u, v in sizes)
    pairs = sum((u - 1) * (v - 1) * c.shape[0] for (u, v), c in zip(sizes, clouds))
    say("grid occupancy of one shape: %d segments, %d cells, %d cloud points, %.2e cell-point pairs; %d repeats after "
        "%d warm-ups, alternating; ms, median [min .. max]" % (a.segments, cells, sum(c.shape[0] for c in clouds),
                                                              pairs, a.repeats, a.warmup))
    medians = {}
    for label, th in (("per-type default thresholds", thres), ("epsilon = 0.1 (test.py)", [0.1] * a.segments)):
        times = {"chamfer": [], "dedicated": []}
        masks = {}
        for r in range(a.warmup + a.repeats):
            for kernel in ("chamfer", "dedicated"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                m = surface.grid_occupancy(grids, sizes, clouds, th, kernel=kernel)
                e1.record()
                e1.synchronize()
                if r >= a.warmup:
                    times[kernel].append(e0.elapsed_time(e1))
                masks[kernel] = m
        same = all(torch.equal(x, y) for x, y in zip(masks["chamfer"], masks["dedicated"]))
        kept = sum(int(x.sum()) for x in masks["dedicated"])
        say("%s: %d of %d cells kept; masks %s" % (label, kept, cells, "identical" if same else "DIFFER"))
        say("    (a) chamfer   (centres + ragged nearest neighbour + compare)  %s" % stats(times["chamfer"]))
        say("    (b) dedicated (one threshold launch)                          %s" % stats(times["dedicated"]))
        medians[label] = (sorted(times["chamfer"])[a.repeats // 2], sorted(times["dedicated"])[a.repeats // 2], same)
    faster = all(d < c and same for c, d, same in medians.values())
    say("(a) / (b): %s -> default PARSENET_TRIM_KERNEL: %s"
        % (", ".join("%.2f" % (c / d) for c, d, _ in medians.values()), "dedicated" if faster else "chamfer"))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
