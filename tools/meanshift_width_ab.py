"""A/B of the mean-shift iterations at embedding widths 32 and 64 (HIP-event timing on torch's current stream).

One forward iteration and one backward iteration at B = 4, N = 10 000, three ways in the same process:
  native   the width kernels (csrc/meanshift_w.hip);
  pad128   the same rows zero-padded to 128 on the 128-wide dense bf16 x 3 launches (no plan);
  tensors  the tensor-library expressions every width but 128 ran before (one shape at a time: it keeps N x N).
The three are timed in alternation, ROUNDS times, REPS calls per timing; printed are the median per variant, the
spread (max - min over the rounds) and, for the native kernels, the executed matrix-core rate: piece products
counted from the shapes (forward 2, row pass 3, column pass 4 GEMM units of 2 N^2 W FLOP per item, six bf16
piece products each) over the kernel time of the launches themselves (pn_prof), against the dense bf16 peak.

A last section probes the width-generic pieces of a clustering call at C = 32, 64 and 128, N = 4 000 and 10 000:
whether kernels.dot_kth_x3 (compute_bandwidth) and kernels.dot_select (compute_bandwidth's exact form, and nms
with k = 1) take their kernel route (they return None outside it), and how far their K-th dot products are from
a tensor-library topk on the same unit rows.

Usage: python tools/meanshift_width_ab.py [--out FILE]"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from parsenet_codebase_amd import _lib, kernels as K

BF16_PEAK_TFLOPS = 2500.0      # dense bf16 matrix peak of the MI355X (MI355X data sheet: 2.5 PFLOP/s)
ROUNDS, REPS, WARMUP = 7, 20, 3


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(REPS):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / REPS


def clustered(B, N, D, seed):
    g = torch.Generator().manual_seed(seed)
    proto = torch.nn.functional.normalize(torch.randn(9, D, generator=g), dim=1)
    x = proto[torch.arange(N) % 9].unsqueeze(0) + 0.3 * torch.randn(B, N, D, generator=g) / np.sqrt(D)
    return torch.nn.functional.normalize(x, dim=2)


def selection_routes(dev):
    out = []
    for C in (32, 64, 128):
        for N in (4000, 10000):
            x = torch.nn.functional.normalize(torch.randn(1, N, C, generator=torch.Generator().manual_seed(C)), dim=2).to(dev)
            kq = int(0.025 * N)
            a = K.dot_kth_x3(x, x, kq)
            b = K.dot_select(x, x, kq, want_value=True)
            c = K.dot_select(x, x, 1, want_value=False)
            ref = torch.topk(x[0] @ x[0].t(), kq, dim=1)[0][:, -1]
            out.append("C=%d N=%d k=%d: dot_kth_x3 %s dot_select(value) %s dot_select(k=1 index) %s; kth max |diff| vs topk: "
                       "x3 %s exact %s"
                       % (C, N, kq, "kernel" if a is not None else "NONE", "kernel" if b is not None else "NONE",
                          "kernel" if c is not None else "NONE",
                          "%.1e" % float((a[0][0] - ref).abs().max()) if a is not None else "-",
                          "%.1e" % float((b[0][0] - ref).abs().max()) if b is not None else "-"))
    return out


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    dev = torch.device("cuda:0")
    B, N = 4, 10000
    lines = ["mean-shift width A/B: B = %d, N = %d, %d rounds x %d calls per variant, alternating; ms per call, "
             "median [min .. max]" % (B, N, ROUNDS, REPS)]
    for W in (32, 64):
        x = clustered(B, N, W, W).to(dev)
        bsq = torch.tensor([0.30, 0.33, 0.36, 0.39], device=dev) ** 2
        gy = torch.randn(B, N, W, generator=torch.Generator().manual_seed(1)).to(dev)
        # native
        wf, wb = K.MeanShiftWWorkspace(B, N, W, dev), K.MeanShiftWWorkspace(B, N, W, dev, backward=True)
        y, r, n = K.meanshift_w_iter_fwd(x, x, bsq, wf)
        gx = torch.zeros_like(x)
        # padded to 128, dense
        xp = torch.nn.functional.pad(x, (0, 128 - W)).contiguous()
        gyp = torch.nn.functional.pad(gy, (0, 128 - W)).contiguous()
        img = K.meanshift_x3_split(xp)
        pf, pb = K.MeanShiftWorkspace(B, N, 128, dev), K.MeanShiftWorkspace(B, N, 128, dev, backward=True, exact_f32=False)
        yp, rp, np_ = K.meanshift_x3_iter_fwd(xp, img, bsq, pf)
        gxp = torch.zeros_like(xp)
        d_fwd = float((yp[..., :W] - y).abs().max())
        gq = K.meanshift_w_iter_bwd(gy, y, x, x, r, n, bsq, wb, gx)
        gqp = K.meanshift_x3_iter_bwd(gyp, yp, xp, xp, img, rp, np_, bsq, pb, gxp)
        d_bwd = float((gqp[..., :W] - gq).abs().max() / gq.abs().max())

        def tensors_fwd():
            for b in range(B):
                Kmat = torch.exp(torch.clamp(-(2.0 - 2.0 * x[b] @ x[b].t()) / bsq[b] / 2, max=75, min=-75))
                u = (Kmat @ x[b]) * (1 / Kmat.sum(1, keepdim=True))
                u / torch.norm(u, dim=1, p=2, keepdim=True)

        def tensors_fwd_bwd():
            for b in range(B):
                xb = x[b].detach().requires_grad_(True)
                Kmat = torch.exp(torch.clamp(-(2.0 - 2.0 * xb @ xb.t()) / bsq[b] / 2, max=75, min=-75))
                u = (Kmat @ xb) * (1 / Kmat.sum(1, keepdim=True))
                ((u / torch.norm(u, dim=1, p=2, keepdim=True)) * gy[b]).sum().backward()
        variants = {
            "fwd native": lambda: K.meanshift_w_iter_fwd(x, x, bsq, wf, out=(y, r, n)),
            "fwd pad128": lambda: K.meanshift_x3_iter_fwd(xp, img, bsq, pf, out=(yp, rp, np_)),
            "fwd tensors": tensors_fwd,
            "bwd native": lambda: K.meanshift_w_iter_bwd(gy, y, x, x, r, n, bsq, wb, gx),
            "bwd pad128": lambda: K.meanshift_x3_iter_bwd(gyp, yp, xp, xp, img, rp, np_, bsq, pb, gxp),
            "fwd+bwd tensors": tensors_fwd_bwd,
        }
        for fn in variants.values():
            for _ in range(WARMUP):
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in variants}
        for _ in range(ROUNDS):
            for k, fn in variants.items():
                t[k].append(timed(fn))
        lines.append("width %d (native against padded-128 on the same rows: iterate max |diff| %.1e, gq rel %.1e)"
                     % (W, d_fwd, d_bwd))
        for k, v in t.items():
            lines.append("  %-16s %8.3f [%8.3f .. %8.3f]" % (k, float(np.median(v)), min(v), max(v)))
        for kind in ("fwd", "bwd"):
            a, p = t[kind + " native"], t[kind + " pad128"]
            lines.append("  %s: native / pad128 = %.3f; spread (max - min) native %.3f ms, pad128 %.3f ms, difference of "
                         "the medians %.3f ms" % (kind, np.median(a) / np.median(p), max(a) - min(a), max(p) - min(p),
                                                  np.median(p) - np.median(a)))
        # kernel times of the native launches and their executed matrix-core rate
        _lib.prof_enable(True)
        _lib.prof_reset()
        for _ in range(REPS):
            K.meanshift_w_iter_fwd(x, x, bsq, wf, out=(y, r, n))
            K.meanshift_w_iter_bwd(gy, y, x, x, r, n, bsq, wb, gx)
        torch.cuda.synchronize()
        pr = {kn: tt / calls for kn, (tt, calls) in _lib.prof_results().items()}
        _lib.prof_enable(False)
        unit = 2.0 * B * float(N) * N * W * 6          # one GEMM unit, six piece products
        for name, units in (("meanshift_w_fwd", 2), ("meanshift_w_bwd_rows", 3), ("meanshift_w_bwd_cols", 4)):
            ms = pr.get(name)
            if ms:
                tf = units * unit / ms / 1e9
                lines.append("  %-22s %.3f ms per launch: %.0f TFLOP/s of bf16 piece products executed = %.2f of the dense "
                             "bf16 peak (%.0f TFLOP/s fp32-equivalent)" % (name, ms, tf, tf / BF16_PEAK_TFLOPS, tf / 6))
    lines.append("")
    lines.append("selection engine at narrow widths (compute_bandwidth: dot_kth_x3; nms: dot_select) on unit rows, one item:")
    lines += selection_routes(dev)
    txt = "\n".join(lines)
    print(txt)
    if out:
        with open(out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
