"""Bit record of the mean-shift iterations on every kernel route, for comparing two commits that must launch the
same kernels in the same order on the same bytes (a change of the host code that drives them).

  python tools/meanshift_routes_dump.py OUT.npz [--label COMMIT]     one process on the GPU: runs the cases below
  python tools/meanshift_routes_dump.py --compare A.npz B.npz [--out FILE]   no GPU: exit status 0 when equal

Every case stores the forward result, the gradient of (y * w).sum() for a fixed seeded w, and
torch.cuda.max_memory_allocated() of the case after reset_peak_memory_stats.  The shapes are the smallest at which
each route can still go wrong; the rows are seeded unit rows drawn around a handful of centres, so that plans skip
tile pairs and Epanechnikov supports hold tens of points.
  dense     B = 2 (two bandwidths), N = 300, iterations 0 / 1 / 3: widths 20, 32, 64, 96, 128 under bf16x3 with both
            kernels; widths 128 and 64 (padded) under f32 and fp16x2; width 64 under PARSENET_MS_NARROW = pad128
  planned   B = 2, N = 2049 and 4100, width 128, 3 iterations, SPARSE on: the autograd backward reuses the plans
  rows      B = 2, N = 4100 and 300, widths 64 and 128, 3 iterations: mean_shift_iterations_state + centre_rows with
            5 rows (one id twice), the gradient through them; the nearest shifted points of the planned call
  auto      B = 2, N = 2049, width 128, SPARSE = "auto", six calls in a row, each reported back like the fitting
            stage does: CALLS and the _AUTO entry after each
Only names that both sides of such a change have are used, so the same file runs on either commit.  The comparison
is equality of every array (shape, dtype, bytes), counter and peak-memory figure: there is no tolerance."""
import gc
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def clustered(B, N, D, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    proto = torch.nn.functional.normalize(torch.randn(B, 5, D, generator=g), dim=2)
    pick = torch.randint(0, 5, (B, N), generator=g)
    x = torch.gather(proto, 1, pick.unsqueeze(2).expand(-1, -1, D)) + 0.2 * torch.randn(B, N, D, generator=g) / np.sqrt(D)
    return torch.nn.functional.normalize(x, dim=2)


def dump(path, label):
    import torch
    from parsenet_codebase_amd import mean_shift as MS
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    rec = {"label": np.array(label)}
    print("package: %s (%s)" % (os.path.dirname(os.path.abspath(MS.__file__)), label), flush=True)
    B = 2

    def case(name, fn, arith="bf16x3", narrow="native", sparse=False):
        """fn() -> dict of tensors / numbers, run under the switches; its peak memory is stored with them."""
        saved = MS.ARITH, MS.NARROW, MS.SPARSE
        MS.ARITH, MS.NARROW, MS.SPARSE = arith, narrow, sparse
        try:
            gc.collect()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            got = fn()
            torch.cuda.synchronize()
            got["peak"] = torch.cuda.max_memory_allocated()
        finally:
            MS.ARITH, MS.NARROW, MS.SPARSE = saved
        for k, v in got.items():
            rec["%s/%s" % (name, k)] = v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
        print("%-44s peak %d" % (name, got["peak"]), flush=True)

    def full(N, D, bw, T, kernel_type):
        def fn():
            x = clustered(B, N, D, 1000 + N + D).to(dev).requires_grad_(True)
            w = torch.randn(B, N, D, generator=torch.Generator().manual_seed(7)).to(dev)
            y = MS.mean_shift_iterations(x, torch.tensor(bw, device=dev), T, kernel_type=kernel_type)
            (y * w).sum().backward()
            return {"y": y, "gx": x.grad}
        return fn

    # ---- dense routes
    for T in (0, 1, 3):
        for D in (20, 32, 64, 96, 128):
            case("dense/bf16x3/gaussian/D%d/T%d" % (D, T), full(300, D, [0.12, 0.2], T, "gaussian"))
            case("dense/bf16x3/epa/D%d/T%d" % (D, T), full(300, D, [0.32, 0.4], T, "epa"))
        for arith in ("f32", "fp16x2"):
            for D in (128, 64):
                case("dense/%s/gaussian/D%d/T%d" % (arith, D, T), full(300, D, [0.12, 0.2], T, "gaussian"), arith=arith)
        case("dense/bf16x3-pad128/gaussian/D64/T%d" % T, full(300, 64, [0.12, 0.2], T, "gaussian"), narrow="pad128")

    # ---- planned route, dense autograd backward on the plans
    for N in (2049, 4100):
        calls = dict(MS.CALLS)
        case("planned/N%d" % N, full(N, 128, [0.1, 0.15], 3, "gaussian"), sparse=True)
        assert MS.CALLS["planned"] == calls["planned"] + 1, "the call was not planned"

    # ---- forward-only state and centre rows
    def rows(N, D):
        def fn():
            x = clustered(B, N, D, 2000 + N + D).to(dev).requires_grad_(True)
            ids = torch.tensor([[3, N - 1, 17, 3, 64], [0, 255, N // 2, 31, 255]], device=dev)
            w = torch.randn(B, 5, D, generator=torch.Generator().manual_seed(8)).to(dev)
            MS.WANT_NEAREST = True
            try:
                new_X, state = MS.mean_shift_iterations_state(x, torch.tensor([0.1, 0.15], device=dev), 3)
            finally:
                MS.WANT_NEAREST = False
            nearest, MS.LAST_NEAREST = MS.LAST_NEAREST, None
            cen = MS.centre_rows(x, state, ids)
            (cen * w).sum().backward()
            got = {"new_X": new_X, "cen": cen, "gx": x.grad}
            if nearest is not None:
                got["nearest"] = nearest
            return got
        return fn
    for N in (4100, 300):
        for D in (64, 128):
            case("rows/N%d/D%d" % (N, D), rows(N, D), sparse=True)

    # ---- auto mode: four probing calls, then dense ones (a bandwidth at which the plans keep everything)
    MS._AUTO.clear()
    for i in range(6):
        def fn():
            got = full(2049, 128, [0.3, 0.35], 3, "gaussian")()
            stat, MS.AUTO_STAT = MS.AUTO_STAT, None
            got["share"] = -1.0 if stat is None else float(stat)
            if stat is not None:
                MS.auto_report(B, 2049, float(stat))
            st = MS._AUTO.get((B, 2049), {"left": -1, "hist": []})
            got["calls"] = [MS.CALLS["planned"], MS.CALLS["dense"]]
            got["auto_left"] = st["left"]
            got["auto_hist"] = np.asarray(st["hist"], dtype=np.float64)
            return got
        case("auto/call%d" % i, fn, sparse="auto")
    np.savez(path, **rec)
    print("wrote %s: %d entries" % (path, len(rec)))


def compare(a_path, b_path, out):
    a, b = np.load(a_path), np.load(b_path)
    lines = ["mean-shift route dump: %s against %s" % (a["label"], b["label"])]
    keys = sorted((set(a.files) | set(b.files)) - {"label"})
    first = None
    for name in sorted({k.rsplit("/", 1)[0] for k in keys}):
        bad = []
        for k in [k for k in keys if k.rsplit("/", 1)[0] == name]:
            if k not in a.files or k not in b.files:
                bad.append(k.rsplit("/", 1)[1] + " (missing)")
                continue
            u, v = a[k], b[k]
            # (bytes: np.array_equal, with a NaN equal to the same NaN and -0.0 not equal to 0.0)
            if u.shape != v.shape or u.dtype != v.dtype or u.tobytes() != v.tobytes():
                bad.append(k.rsplit("/", 1)[1])
        lines.append("%-44s %s" % (name, "equal" if not bad else "DIFFERENT: " + ", ".join(bad)))
        if bad and first is None:
            first = name
    lines.append("equal: every array, counter and peak-memory figure" if first is None
                 else "first differing case: %s" % first)
    txt = "\n".join(lines)
    print(txt)
    if out:
        with open(out, "w") as fh:
            fh.write(txt + "\n")
    return 0 if first is None else 1


if __name__ == "__main__":
    argv = sys.argv[1:]
    if argv and argv[0] == "--compare":
        sys.exit(compare(argv[1], argv[2], argv[argv.index("--out") + 1] if "--out" in argv else None))
    if not argv:
        sys.exit(__doc__)
    dump(argv[0], argv[argv.index("--label") + 1] if "--label" in argv else "unlabelled")
