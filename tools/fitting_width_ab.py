"""A/B of the training-mode fitting stage at embedding widths 50 and 64 (HIP events on torch's current stream and
the host's wall clock, forward + backward of one stage call).

The batch is cfg5's synthetic one — 4 shapes of 10 000 points (synthetic.make_batch(0, 4, 10000)) — with a
structured embedding of the asked width: one random unit code per ground-truth segment plus noise of the norm the
128-wide stage tests use (0.035 sqrt(128) whatever the width).  Three cases, alternating in one process:
  native     this tree: the stage batched at the kernels' width (50 -> 64, 64 as it is);
  pad128     this tree with PARSENET_MS_NARROW=pad128: the stage batched at width 128 (block-sparse plans, the
             locality order and the nearest-point by-product included);
  per-shape  what the parent commit ran at these widths: every shape alone through ev.guard_mean_shift (one
             host synchronisation per shape, dense backward through all N rows), memberships as bmm + tensor
             expressions.  Reproduced here by closing the two gates the parent had closed (bandwidth_batch -> None,
             MEMBERSHIP_WIDTHS -> (128,)); with ``--parent-tree DIR`` (an export of the parent commit, built) the
             same measurement is also taken by a child process that imports the package from DIR.
Printed per case: median [min .. max] over ROUNDS timed calls after WARMUP untimed ones, the loss (so the cases
can be seen to compute the same thing) and how many shapes took which path (fitting_batch.CALLS_STAGE).

Usage: python tools/fitting_width_ab.py [--out FILE] [--parent-tree DIR]"""
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
TREE = sys.argv[sys.argv.index("--tree") + 1] if "--tree" in sys.argv else os.path.dirname(HERE)
sys.path.insert(0, TREE)
import numpy as np
import torch

ROUNDS, WARMUP = 7, 2
WIDTHS = (50, 64)


def batch(W, dev):
    from parsenet_codebase_amd import synthetic
    B, N = 4, 10000
    pts, nrm, lab, prim = synthetic.make_batch(0, B, N)
    g = torch.Generator().manual_seed(99)
    code = torch.nn.functional.normalize(torch.randn(64, W, generator=g), dim=1)
    per = 0.035 * float(np.sqrt(128.0 / W))
    emb = torch.nn.functional.normalize(code[torch.from_numpy(lab).long()] + per * torch.randn(B, N, W, generator=g), dim=2)
    logp = torch.log_softmax(torch.randn(B, 10, N, generator=g), 1)
    return (torch.from_numpy(pts).to(dev), torch.from_numpy(nrm).to(dev), lab, prim, emb.to(dev), logp.to(dev))


def evaluation(dev):
    from parsenet_codebase_amd.encoders import DGCNNControlPoints
    from parsenet_codebase_amd.fitting import Evaluation
    torch.manual_seed(0)
    return Evaluation(closed_path=DGCNNControlPoints(20, num_points=10, mode=1).to(dev),
                      open_path=DGCNNControlPoints(20, num_points=10, mode=0).to(dev))


def one_call(ev, data):
    """One stage forward + backward: (HIP-event ms, wall ms, loss)."""
    P, Nn, lab, prim, emb, logp = data
    e = emb.clone().requires_grad_(True)
    np.random.seed(5)
    torch.cuda.synchronize()
    s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    s.record()
    res = ev.fitting_losses(e, P, Nn, lab, prim, logp, quantile=0.025, iterations=10, lamb=0.1)
    loss = sum(r[0][0].sum() for r in res)
    loss.backward()
    t.record()
    torch.cuda.synchronize()
    return s.elapsed_time(t), (time.perf_counter() - t0) * 1e3, float(loss)


def fmt(v):
    return "%8.2f [%8.2f .. %8.2f]" % (float(np.median(v)), min(v), max(v))


def parent_only(dev):
    """Child-process mode (--only-parent): the stage as the tree at --tree runs it, one JSON line per width."""
    ev = evaluation(dev)
    for W in WIDTHS:
        data = batch(W, dev)
        for _ in range(WARMUP):
            one_call(ev, data)
        runs = [one_call(ev, data) for _ in range(ROUNDS)]
        print(json.dumps({"width": W, "gpu_ms": [r[0] for r in runs], "wall_ms": [r[1] for r in runs], "loss": runs[-1][2]}))


def main():
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    if "--only-parent" in sys.argv:
        return parent_only(dev)
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    parent = sys.argv[sys.argv.index("--parent-tree") + 1] if "--parent-tree" in sys.argv else None
    from parsenet_codebase_amd import fitting_batch as FB, mean_shift as MSM
    ev = evaluation(dev)
    real_bandwidth, real_widths, real_narrow = FB.bandwidth_batch, FB.MEMBERSHIP_WIDTHS, MSM.NARROW

    def setup(case):
        MSM.NARROW = "pad128" if case == "pad128" else "native"
        FB.bandwidth_batch = (lambda *a, **k: None) if case == "per-shape" else real_bandwidth
        FB.MEMBERSHIP_WIDTHS = (128,) if case == "per-shape" else real_widths
    cases = ("native", "pad128", "per-shape")
    lines = ["fitting stage width A/B: 4 shapes x 10 000 points, forward + backward of one stage call, %d timed calls per "
             "case after %d untimed, cases alternating; ms per call, median [min .. max]" % (ROUNDS, WARMUP)]
    try:
        for W in WIDTHS:
            data = batch(W, dev)
            for case in cases:
                setup(case)
                for _ in range(WARMUP):
                    one_call(ev, data)
            t = {c: [] for c in cases}
            took = {}
            for _ in range(ROUNDS):
                for case in cases:
                    setup(case)
                    before = dict(FB.CALLS_STAGE)
                    t[case].append(one_call(ev, data))
                    took[case] = {k: FB.CALLS_STAGE[k] - before[k] for k in before}
            lines.append("width %d (kernels' width %d)" % (W, MSM.kernel_width(W)))
            for case in cases:
                lines.append("  %-10s GPU timeline %s   wall %s   loss %.6f   shapes batched / per shape: %d / %d"
                             % (case, fmt([r[0] for r in t[case]]), fmt([r[1] for r in t[case]]), t[case][-1][2],
                                took[case]["batched"], took[case]["per_shape"]))
            med = {c: float(np.median([r[1] for r in t[c]])) for c in cases}
            lines.append("  wall: native / pad128 = %.3f, native / per-shape = %.3f, pad128 / per-shape = %.3f"
                         % (med["native"] / med["pad128"], med["native"] / med["per-shape"], med["pad128"] / med["per-shape"]))
    finally:
        FB.bandwidth_batch, FB.MEMBERSHIP_WIDTHS, MSM.NARROW = real_bandwidth, real_widths, real_narrow
    if parent:
        # a fresh child process (this one has initialised the GPU): the parent commit's own code on the same batch
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--tree", os.path.abspath(parent), "--only-parent"],
                           capture_output=True, text=True, timeout=900)
        lines.append("parent commit's tree (%s), child process, after this process's cases:" % os.path.basename(os.path.abspath(parent)))
        if r.returncode != 0:
            lines.append("  child failed (exit %d): %s" % (r.returncode, r.stderr.strip().splitlines()[-1:] or ""))
        for ln in r.stdout.splitlines():
            if ln.startswith("{"):
                d = json.loads(ln)
                lines.append("  width %d  GPU timeline %s   wall %s   loss %.6f" % (d["width"], fmt(d["gpu_ms"]), fmt(d["wall_ms"]), d["loss"]))
    txt = "\n".join(lines)
    print(txt)
    if out:
        with open(out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
