"""Timing of the dominant-plane extraction (csrc/plane.hip) beside the host route a user has without it.

    python tools/plane_ab.py [--out profiles/plane.txt] [--reps 20] [--limit 300]

Sizes: 10 000, 100 000 and 1 000 000 points and a batch of 4 x 10 000.  Each cloud is a jittered plane that carries
about 60 % of the points with the five jittered tori of tools/cluster_ab.py (R = 1, r = 0.3, four apart) standing on
it; the clouds of a batch have different seeds.  The threshold is three times the jitter of the plane, H = 512,
refine = 1.  The parent starts one child process per size under its own time limit and stops at the first that fails; a
child makes two warm-up calls and then times ``kernels.plane_ragged`` (every output) with HIP events, median of --reps
runs, and prints the launches, the inliers it found, the time per point and hypothesis, and the share of the scoring
launch in the whole call (the library's own HIP-event spans "plane" and "plane_score", over five further calls).
Beside it, alternating in the same run:
  host route  download, the same definition in numpy (every hypothesis against every point in fp64, chunks of
              hypotheses, the winner refined once by numpy.linalg.eigh), upload of the mask; wall clock, HOST_RUNS runs
              spread between the timed calls.  Its refit sums in another order, so only the inlier count is compared."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(10000, 1), (100000, 1), (1000000, 1), (10000, 4)]
TORI, SHARE, H, REFINE = 5, 0.6, 512, 1
AREA = 4 * 3.141592653589793 ** 2 * 1.0 * 0.3
HOST_RUNS = 3
M64 = (1 << 64) - 1


def scene(n, seed):
    """(n,3) fp32 and the threshold: a jittered plane under five jittered tori, shuffled."""
    import numpy as np
    rng = np.random.RandomState(seed)
    flat = int(n * SHARE)
    per = (n - flat) // TORI
    spacing = (AREA / per) ** 0.5
    jitter = 0.1 * spacing
    parts = [np.stack([rng.uniform(-2, 18, flat), rng.uniform(-2, 2, flat), jitter * rng.normal(size=flat)], 1)]
    for t in range(TORI):
        m = per if t else n - flat - per * (TORI - 1)
        u, v = rng.uniform(0, 2 * np.pi, (2, m))
        P = np.stack([(1 + 0.3 * np.cos(v)) * np.cos(u), (1 + 0.3 * np.cos(v)) * np.sin(u), 0.3 * np.sin(v)], 1)
        parts.append(P + jitter * rng.normal(size=P.shape) + np.asarray([4.0 * t, 0.0, 0.3]))
    P = np.concatenate(parts).astype(np.float32)
    return P[rng.permutation(n)], float(np.float32(3 * jitter))


def _mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def host_route(torch, pts, t, seed=0, chunk=32):
    """One cloud on the GPU -> (mask on the GPU, inliers), by numpy on the host."""
    import numpy as np
    X = pts.cpu().numpy().astype(np.float64)
    n = X.shape[0]
    idx = np.asarray([[((_mix((seed + 0x9E3779B97F4A7C15 * (3 * h + s + 1)) & M64) >> 32) * n) >> 32 for s in range(3)]
                      for h in range(H)])
    p0 = X[idx[:, 0]]
    c = np.cross(X[idx[:, 1]] - p0, X[idx[:, 2]] - p0)
    length = np.linalg.norm(c, axis=1)
    ok = (length > 0) & (idx[:, 0] != idx[:, 1]) & (idx[:, 0] != idx[:, 2]) & (idx[:, 1] != idx[:, 2])
    nrm = c / np.where(ok, length, 1.0)[:, None]
    d = -(nrm * p0).sum(1)
    counts = np.zeros(H, np.int64)
    for h0 in range(0, H, chunk):
        counts[h0:h0 + chunk] = (np.abs(nrm[h0:h0 + chunk] @ X.T + d[h0:h0 + chunk, None]) <= t).sum(1)
    best = int(np.argmax(np.where(ok, counts, -1)))
    inl = np.abs(X @ nrm[best] + d[best]) <= t
    for _ in range(REFINE):
        mean = X[inl].mean(0)
        w, v = np.linalg.eigh(np.cov((X[inl] - mean).T))
        again = np.abs((X - mean) @ v[:, 0]) <= t
        if again.sum() < inl.sum():
            break
        inl = again
    out = torch.from_numpy(inl).to(pts.device)
    torch.cuda.synchronize()
    return out, int(inl.sum())


def _timed(torch, fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    out = fn()
    t1.record()
    torch.cuda.synchronize()
    return out, t0.elapsed_time(t1)


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
    thr = torch.tensor([c[1] for c in clouds], dtype=torch.float32, device=pts.device)

    def ours():
        return kernels.plane_ragged(flat, off, thr, H, 0, REFINE)

    def theirs():
        return [host_route(torch, pts[b], clouds[b][1]) for b in range(batch)]

    ref = _timed(torch, ours)[0]
    assert all(torch.equal(a, b) for a, b in zip(ref, _timed(torch, ours)[0])), "a second run changed a result"
    t, th = [], []
    host_at = set(int(v) for v in np.linspace(0, reps - 1, HOST_RUNS))
    for rep in range(reps):                                      # the competitors alternate in one run
        t.append(_timed(torch, ours)[1])
        if rep in host_at:
            w0 = time.perf_counter()
            other = theirs()
            th.append(1e3 * (time.perf_counter() - w0))
    t, th = np.asarray(t), np.asarray(th)
    _lib.prof_reset()
    _lib.prof_enable(True)
    for _ in range(5):
        ours()
    torch.cuda.synchronize()
    spans = {name: ms for name, (ms, _) in _lib.prof_results().items()}
    _lib.prof_enable(False)
    share = spans.get("plane_score", float("nan")) / spans.get("plane", float("nan"))
    count = ref[1].tolist()
    found = [o[1] for o in other]
    line = ("%d x %d points, threshold %.5f, H %d, refine %d -> %s inliers (best %s): %d launches, workspace %.2f MB, "
            "median %.3f ms (min %.3f, max %.3f), %.3f ns per point, %.2f ps per point and hypothesis; the scoring "
            "launch is %.0f %% of the call; %d runs; host route (download, numpy in chunks of hypotheses, upload), wall "
            "clock, same run, %d runs: median %.1f ms (min %.1f, max %.1f): %.1f times the kernels' time; it found %s "
            "inliers"
            % (batch, n, clouds[0][1], H, REFINE, " + ".join(str(v) for v in count),
               " + ".join(str(v) for v in ref[2].tolist()), lib.pn_plane_launches(REFINE),
               lib.pn_plane_workspace_bytes(batch * n, batch, H) / 1e6, np.median(t), t.min(), t.max(),
               1e6 * np.median(t) / (batch * n), 1e9 * np.median(t) / (batch * n * H), 100 * share, reps, len(th),
               np.median(th), th.min(), th.max(), np.median(th) / np.median(t), " + ".join(str(v) for v in found)))
    print(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plane.txt"))
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
        f.write("tools/plane_ab.py: MI355X, %d timed runs per size after two warm-up runs, HIP events; plane, count, "
                "best, inlier and dist, H = %d, refine = %d\n" % (args.reps, H, REFINE))
        f.write("".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
