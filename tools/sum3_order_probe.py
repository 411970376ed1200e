"""In which order does the tensor library's GPU reduction add the three squares of torch.sum((a - b) ** 2, 2)?
chamfer.nn_sqdist reports that expression at the Chamfer kernel's arg-min, and csrc/cover.hip has to reproduce its
last bit.  For (1, M, 3) fp32 inputs in the unit box and M from 1 to 100 000 the GPU result is compared bit for bit
with every candidate evaluated in numpy on the host: the three association orders of the rounded squares, and for
each order the two contracted forms (one or two fused multiply-adds, emulated in float64: a product of two fp32 is
exact there, the one rounding of the sum to fp64 before the rounding to fp32 can differ from a real fma only in a
double-rounding case, which a candidate would show as a handful of mismatches, not as zero).

    python tools/sum3_order_probe.py --out profiles/sum3_order.txt
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def candidates(d):
    """d (M,3) fp32 differences -> {name: (M,) fp32}"""
    f32, f64 = np.float32, np.float64
    sq = (d * d).astype(f32)
    out = {}
    for name, (i, j, k) in (("(x+y)+z", (0, 1, 2)), ("(x+z)+y", (0, 2, 1)), ("(y+z)+x", (1, 2, 0))):
        out[name] = ((sq[:, i] + sq[:, j]).astype(f32) + sq[:, k]).astype(f32)
        di, dj, dk = d[:, i].astype(f64), d[:, j].astype(f64), d[:, k].astype(f64)
        inner = (sq[:, i] + sq[:, j]).astype(f32)
        out[name + ", outer fma"] = (dk * dk + inner.astype(f64)).astype(f32)
        inner = (dj * dj + sq[:, i].astype(f64)).astype(f32)
        out[name + ", two fma"] = (dk * dk + inner.astype(f64)).astype(f32)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/sum3_order.txt")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("torch %s on %s: rows of torch.sum((a - b) ** 2, 2), a and b (1, M, 3) fp32, that differ in any bit from the "
        "candidate" % (torch.__version__, torch.cuda.get_device_name(dev)))
    rng = np.random.RandomState(5)
    sizes = (1, 2, 3, 7, 64, 300, 930, 1237, 10000, 100000)
    total = {}
    for m in sizes:
        x = rng.uniform(-0.5, 0.5, (1, m, 3)).astype(np.float32)
        y = rng.uniform(-0.5, 0.5, (1, m, 3)).astype(np.float32)
        got = torch.sum((torch.from_numpy(x).to(dev) - torch.from_numpy(y).to(dev)) ** 2, 2).cpu().numpy()[0]
        d = (x - y)[0]                                     # one rounding, as on the device
        row = []
        for name, want in candidates(d).items():
            bad = int((got.view(np.int32) != want.view(np.int32)).sum())
            total[name] = total.get(name, 0) + bad
            row.append("%s: %d" % (name, bad))
        say("M = %6d  %s" % (m, "; ".join(row)))
    exact = [n for n, bad in total.items() if bad == 0]
    say("candidates that reproduce every row at every size: %s" % (", ".join(exact) if exact else "none"))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
