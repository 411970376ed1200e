"""A/B of mean-shift with the Epanechnikov kernel: the fused kernels against the tensor expressions.

One clustering-sized call — N = 10 000 unit rows, ten iterations, forward + backward through
MeanShift.mean_shift_(kernel_type="epa") — at embedding widths 64 and 128, two ways in the same process:
  fused    the Epanechnikov form of the fused, recompute-backward kernels (csrc/meanshift_w.hip at width 64,
           csrc/meanshift_x3.h dense launches at width 128; PARSENET_MS_ARITH = bf16x3, the default);
  tensors  the tensor-library expressions the call ran before and still runs under the other arithmetics
           (they keep the N x N kernel matrix of every iteration for autograd).
The two are timed in alternation with HIP events on torch's current stream, ROUNDS times, REPS calls per
timing, after WARMUP calls each; printed are the median per variant and its range over the rounds, the peak
rise of the caching allocator over one call of each (against 4 N^2 bytes, one N x N fp32 matrix), and how far
the two results are apart.

Usage: python tools/meanshift_epa_ab.py [--out FILE]"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from parsenet_codebase_amd import mean_shift as MSM

ROUNDS, REPS, WARMUP = 5, 3, 2
N, ITERATIONS, BANDWIDTH = 10000, 10, 0.3


def clustered(N, D, seed):
    g = torch.Generator().manual_seed(seed)
    proto = torch.nn.functional.normalize(torch.randn(9, D, generator=g), dim=1)
    x = proto[torch.randint(0, 9, (N,), generator=g)] + 0.2 * torch.randn(N, D, generator=g) / np.sqrt(D)
    return torch.nn.functional.normalize(x, dim=1)


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(REPS):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / REPS


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    lines = ["mean-shift Epanechnikov A/B: N = %d, %d iterations forward + backward, b = %.2f, %d rounds x %d calls "
             "per variant, alternating; ms per call, median [min .. max]" % (N, ITERATIONS, BANDWIDTH, ROUNDS, REPS)]
    for W in (64, 128):
        x = clustered(N, W, W).to(dev)
        w = torch.randn(N, W, generator=torch.Generator().manual_seed(4)).to(dev)
        b = torch.tensor(BANDWIDTH, device=dev)
        res = {}

        def call(arith):
            old, MSM.ARITH = MSM.ARITH, arith
            try:
                xg = x.clone().requires_grad_(True)
                y, _ = MSM.MeanShift().mean_shift_(xg, b, ITERATIONS, kernel_type="epa")
                (y * w).sum().backward()
                res[arith] = (y.detach(), xg.grad)
            finally:
                MSM.ARITH = old
        variants = {"fused": lambda: call("bf16x3"), "tensors": lambda: call("f32")}
        peak = {}
        for k, fn in variants.items():
            for _ in range(WARMUP):
                fn()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            before = MSM.CALLS_EPA
            fn()
            torch.cuda.synchronize()
            peak[k] = torch.cuda.max_memory_allocated() - base
            assert (MSM.CALLS_EPA == before + 1) == (k == "fused"), "the variant did not take its path"
        (yf, gf), (yt, gt) = res["bf16x3"], res["f32"]
        t = {k: [] for k in variants}
        for _ in range(ROUNDS):
            for k, fn in variants.items():
                t[k].append(timed(fn))
        lines.append("width %d (fused against tensors: iterate max |diff| %.1e, gradient rel %.1e)"
                     % (W, float((yf - yt).abs().max()), float((gf - gt).abs().max() / gt.abs().max())))
        for k, v in t.items():
            lines.append("  %-8s %9.3f [%9.3f .. %9.3f] ms   peak rise %9.1f MB = %6.2f N x N fp32 matrices"
                         % (k, float(np.median(v)), min(v), max(v), peak[k] / 1e6, peak[k] / (4.0 * N * N)))
        a, p = t["fused"], t["tensors"]
        lines.append("  fused / tensors = %.3f in time (spread max - min: fused %.3f ms, tensors %.3f ms), %.4f in peak "
                     "memory" % (np.median(a) / np.median(p), max(a) - min(a), max(p) - min(p),
                                 peak["fused"] / peak["tensors"]))
    txt = "\n".join(lines)
    print(txt)
    if out:
        with open(out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
