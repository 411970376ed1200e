"""Timing of the voxel-grid downsampling (csrc/voxel.hip) beside the same definition written as tensor expressions, and
of the pipeline it was built for: voxel grid first, farthest-point sampling on what is left.

    python tools/voxel_ab.py [--out profiles/voxel.txt] [--reps 20] [--limit 300]

Sizes: 10 000, 100 000 and 1 000 000 points and a batch of 4 x 10 000, each cloud a jittered torus
(tools/orient_normals_ab.py), the clouds of a batch with different seeds; the voxel size leaves about a tenth of the
points (VOXEL_PER_POINT).  The parent starts one child process per size under its own time limit and stops at the first
that fails; a child makes two warm-up calls and then times ``kernels.voxel_ragged`` (every output) with HIP events,
median of --reps runs, and prints the launches, the voxels it found and the time per point.  Beside it:
  tensor expressions  on the GPU, per cloud: fp64 cells, one 63-bit integer key per point, ``torch.unique`` with
              ``return_inverse``, ``index_add_`` of the fp64 coordinates and of ones, a division.  Voxels come out in
              key order and the sums in torch's order, so only the number of voxels is compared.  HIP events, the same
              number of runs.
The last child times the pipeline on 1 000 000 points: ``voxel_downsample`` (position="point") to about 100 000 points
followed by ``reduce_cloud(..., 10000)``, against ``reduce_cloud(..., 10000)`` alone on the 1 000 000 points — both in
the same process, alternating, each including its host reads."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(10000, 1), (100000, 1), (1000000, 1), (10000, 4)]
PIPELINE = (1000000, 10000)
# The torus has an area of 6.9; its points fall into about 1.6 area / h^2 cells of edge h while the cells are far
# smaller than the tube and hold several points each.  h = VOXEL_PER_POINT / sqrt(n) leaves about n / 10 voxels.
VOXEL_PER_POINT = 9.5


def voxel_size(n):
    return VOXEL_PER_POINT / n ** 0.5


def torch_voxels(P, h):
    """(N,3) fp32 -> (centroid (V,3) fp32, count (V), inverse (N)): the tensor expressions a user would write."""
    import torch
    lo = P.min(0).values.double()
    cell = torch.floor((P.double() - lo) / h).long()
    key = (cell[:, 0] << 42) | (cell[:, 1] << 21) | cell[:, 2]
    _, inverse = torch.unique(key, return_inverse=True)
    V = int(inverse.max()) + 1
    sums = torch.zeros((V, 3), dtype=torch.float64, device=P.device).index_add_(0, inverse, P.double())
    count = torch.bincount(inverse, minlength=V)
    return (sums / count[:, None]).float(), count, inverse


def _timed(torch, fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    out = fn()
    t1.record()
    torch.cuda.synchronize()
    return out, t0.elapsed_time(t1)


def _clouds(n, batch):
    import numpy as np
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from orient_normals_ab import jittered_torus
    return np.stack([jittered_torus(n, seed=4 + b)[0] for b in range(batch)])


def child(n, batch, reps):
    import numpy as np
    import torch
    host = _clouds(n, batch)
    from parsenet_codebase_amd import _lib, kernels
    lib = _lib.load()
    pts = torch.from_numpy(host).cuda()
    flat = pts.reshape(-1, 3)
    off = torch.arange(batch + 1, dtype=torch.int32, device=pts.device) * n
    h = voxel_size(n)
    vox = torch.full((batch,), h, dtype=torch.float32, device=pts.device)

    def ours():
        return kernels.voxel_ragged(flat, off, vox)

    def theirs():
        return [torch_voxels(pts[b], float(np.float32(h))) for b in range(batch)]

    ref = _timed(torch, ours)[0]
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32))                              # (bits: NaN rows)
               for a, b in zip(ref, _timed(torch, ours)[0])), "a second run changed a result"      # two warm-ups
    t = np.asarray([_timed(torch, ours)[1] for _ in range(reps)])
    for _ in range(2):
        other = _timed(torch, theirs)[0]
    tt = np.asarray([_timed(torch, theirs)[1] for _ in range(reps)])
    nvox = ref[1].tolist()
    assert nvox == [o[0].shape[0] for o in other], "the tensor expressions found other voxels"
    print("%d x %d points, voxel %.5f -> %s voxels: %d launches, workspace %.1f MB, median %.3f ms (min %.3f, max %.3f), "
          "%.2f ns per point; %d runs; tensor expressions on the GPU median %.3f ms (min %.3f, max %.3f): %.2f times the "
          "kernels' time"
          % (batch, n, h, " + ".join(str(v) for v in nvox), lib.pn_voxel_launches(),
             lib.pn_voxel_workspace_bytes(batch * n, batch) / 1e6, np.median(t), t.min(), t.max(),
             1e6 * np.median(t) / (batch * n), reps, np.median(tt), tt.min(), tt.max(), np.median(tt) / np.median(t)))


def pipeline(n, m, reps):
    import numpy as np
    import torch
    host = _clouds(n, 1)[0]
    from parsenet_codebase_amd.sampling import lift, reduce_cloud, voxel_downsample
    pts = torch.from_numpy(host).cuda()
    h = voxel_size(n)

    def composed():
        vox, own_v = voxel_downsample(pts, h, position="point")
        red, own_f = reduce_cloud(vox, m)
        return red, own_f, own_v, vox.shape[0]

    def voxel_only():
        return voxel_downsample(pts, h, position="point")

    def alone():
        return reduce_cloud(pts, m)

    for _ in range(2):
        red, own_f, own_v, V = _timed(torch, composed)[0]
        _timed(torch, voxel_only)
        _timed(torch, alone)
    labels = lift(lift(torch.arange(m, device=pts.device), own_f), own_v)
    assert labels.shape[0] == n and int(labels.max()) == m - 1
    tc, tv, ta = [], [], []
    for _ in range(reps):                                        # alternating, in one process
        tc.append(_timed(torch, composed)[1])
        tv.append(_timed(torch, voxel_only)[1])
        ta.append(_timed(torch, alone)[1])
    tc, tv, ta = (np.asarray(x) for x in (tc, tv, ta))
    print("pipeline on %d points: voxel_downsample (voxel %.5f, position=\"point\") -> %d points, then reduce_cloud -> %d "
          "samples: median %.2f ms (min %.2f, max %.2f), of which voxel_downsample with its host read %.2f ms; "
          "reduce_cloud alone on the %d points, same run: median %.2f ms (min %.2f, max %.2f); the composed pipeline "
          "takes %.2f times the time of the sampling alone; %d runs each, alternating"
          % (n, h, V, m, np.median(tc), tc.min(), tc.max(), np.median(tv), n, np.median(ta), ta.min(), ta.max(),
             np.median(tc) / np.median(ta), reps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxel.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--limit", type=int, default=300, help="seconds per size")
    ap.add_argument("--child", nargs=2, type=int, metavar=("N", "BATCH"))
    ap.add_argument("--pipeline", nargs=2, type=int, metavar=("N", "M"))
    args = ap.parse_args()
    if args.child:
        child(args.child[0], args.child[1], args.reps)
        return 0
    if args.pipeline:
        pipeline(args.pipeline[0], args.pipeline[1], args.reps)
        return 0
    jobs = [["--child", str(n), str(batch)] for n, batch in SIZES] + [["--pipeline"] + [str(v) for v in PIPELINE]]
    lines = []
    for job in jobs:
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
        f.write("tools/voxel_ab.py: MI355X, %d timed runs per size after two warm-up runs, HIP events; owner, nvox, "
                "centroid, count, first and rep\n" % args.reps)
        f.write("".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
