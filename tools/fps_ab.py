"""Timing of the farthest-point sampling (csrc/fps.hip) beside the two ways there were to do it without the kernel.

    python tools/fps_ab.py [--out profiles/fps.txt] [--reps 20] [--limit 300]

Sizes (points -> samples): 10 000 -> 2 500, 100 000 -> 10 000, 1 000 000 -> 10 000 and a batch of 4 x 10 000 -> 2 500,
each cloud a jittered torus (tools/orient_normals_ab.py), the clouds of a batch with different seeds.  The parent starts
one child process per size under its own time limit and stops at the first that fails; a child makes two warm-up calls
and then times ``kernels.fps_ragged`` (sample, owner, dist and radius) with HIP events, median of --reps runs, and
prints the launch count, the time per step, and the bytes a step has to move (16 per point: the row and D) over that
time; the record ends with the time per step at 10 000 beside 100 000 points, which tells a launch-bound step.  Beside
it:
  torch loop  on the GPU: distance to the last sample, ``minimum``, ``argmax``, no host read inside the loop; HIP events,
              the same number of runs.  Its sum order is torch's, so its samples may differ from the kernel's: the length
              of the common prefix is a figure, not an assertion.
  numpy loop  on the host, wall clock, one run; at 1 000 000 points 100 steps only, the total EXTRAPOLATED from the
              time per step."""
import argparse
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(10000, 2500, 1), (100000, 10000, 1), (1000000, 10000, 1), (10000, 2500, 4)]
NUMPY_FULL_UP_TO = 100000      # above it the numpy loop runs NUMPY_STEPS steps and is extrapolated
NUMPY_STEPS = 100


def torch_fps(P, m):
    """(B,N,3) -> (B,m) samples: the loop a user would write with torch alone."""
    import torch
    B, N, _ = P.shape
    D = torch.full((B, N), float("inf"), device=P.device)
    sel = torch.zeros(B, dtype=torch.long, device=P.device)
    rows = torch.arange(B, device=P.device)
    out = torch.empty((B, m), dtype=torch.long, device=P.device)
    for t in range(m):
        out[:, t] = sel
        d = ((P - P[rows, sel][:, None, :]) ** 2).sum(-1)
        D = torch.minimum(D, d)
        sel = D.argmax(1)
    return out


def numpy_fps(P, steps):
    """(N,3) -> samples of ``steps`` steps, float32."""
    import numpy as np
    D = np.full(P.shape[0], np.inf, np.float32)
    out = np.empty(steps, np.int64)
    s = 0
    for t in range(steps):
        out[t] = s
        d = ((P - P[s]) ** 2).sum(-1)
        D = np.minimum(D, d)
        s = int(D.argmax())
    return out


def child(n, m, batch, reps):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from orient_normals_ab import jittered_torus
    from parsenet_codebase_amd import _lib, kernels
    lib = _lib.load()
    host = np.stack([jittered_torus(n, seed=4 + b)[0] for b in range(batch)])
    pts = torch.from_numpy(host).cuda()
    flat = pts.reshape(-1, 3)
    off = torch.arange(batch + 1, dtype=torch.int32, device=pts.device) * n

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = fn()
        t1.record()
        torch.cuda.synchronize()
        return out, t0.elapsed_time(t1)

    def ours():
        return kernels.fps_ragged(flat, off, n, m, want_owner=True, want_radius=True)

    ref = timed(ours)[0]
    assert all(torch.equal(a, b) for a, b in zip(ref, timed(ours)[0])), "a second run changed a result"   # two warm-ups
    t = np.asarray([timed(ours)[1] for _ in range(reps)])
    for _ in range(2):
        other = timed(lambda: torch_fps(pts, m))[0]
    tt = np.asarray([timed(lambda: torch_fps(pts, m))[1] for _ in range(reps)])
    same = (other == ref[0].long()).to(torch.uint8).cumprod(1).sum(1).min().item()
    steps = m if n <= NUMPY_FULL_UP_TO else NUMPY_STEPS
    w0 = time.perf_counter()
    for b in range(batch):
        numpy_fps(host[b], steps)
    wall = 1e3 * (time.perf_counter() - w0)
    step_us = 1e3 * np.median(t) / m
    gbs = 16.0 * batch * n / (step_us * 1e-6) / 1e9
    line = ("%d x %d points -> %d samples: %d launches, median %.3f ms (min %.3f, max %.3f), %.2f us per step, a step "
            "moves %.0f KB: %.0f GB/s; %d runs; torch loop on the GPU median %.1f ms (min %.1f), %.1f us per step, the "
            "first %d samples the same; "
            % (batch, n, m, lib.pn_fps_launches(m), np.median(t), t.min(), t.max(), step_us, 16e-3 * batch * n, gbs,
               reps, np.median(tt), tt.min(), 1e3 * np.median(tt) / m, same))
    if steps == m:
        line += "numpy loop on the host %.0f ms (wall clock, 1 run)" % wall
    else:
        line += ("numpy loop on the host %.2f ms per step over %d steps: %.0f ms for %d steps, EXTRAPOLATED"
                 % (wall / steps, steps, wall / steps * m, m))
    print(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fps.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--limit", type=int, default=300, help="seconds per size")
    ap.add_argument("--child", nargs=3, type=int, metavar=("N", "M", "BATCH"))
    args = ap.parse_args()
    if args.child:
        child(args.child[0], args.child[1], args.child[2], args.reps)
        return 0
    lines = []
    for n, m, batch in SIZES:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", str(n),
               str(m), str(batch), "--reps", str(args.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        lines.append(r.stdout)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            print("size (%d points, %d samples, batch %d) ended with status %d: stopping" % (n, m, batch, r.returncode))
            return r.returncode
    per_step = [float(re.search(r"([0-9.]+) us per step", text).group(1)) for text in lines]
    with open(args.out, "w") as f:
        f.write("tools/fps_ab.py: MI355X, %d timed runs per size after two warm-up runs, HIP events; sample, owner, "
                "dist and radius; m + 2 launches\n" % args.reps)
        f.write("".join(lines))
        f.write("per step: %.2f us at %d points, %.2f us at %d: %d times the points in %.2f times the time"
                % (per_step[0], SIZES[0][0], per_step[1], SIZES[1][0], SIZES[1][0] // SIZES[0][0],
                   per_step[1] / per_step[0]))
        if per_step[1] < 2 * per_step[0]:
            f.write(" - at %d points the step is dominated by the fixed cost of a launch (and of the dependent chain "
                    "slot -> row -> key -> atomic behind it), not by the points: the measured case for a one-workgroup "
                    "engine with the cloud in registers, which this kernel is not" % SIZES[0][0])
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
