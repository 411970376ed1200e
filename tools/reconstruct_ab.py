"""A/B of the reconstruction metrics of a batch of shapes: (a) test.py's loop, shape by shape on the per-segment entry
— np.random.seed, residual_eval_mode(sample_points=True, if_visualize=True), sample_from_collection_of_mesh,
coverage_metrics, SIOU_matched_segments — against (b) fitting_eval.reconstruct_batch on the same shapes and seeds.

    python tools/reconstruct_ab.py       (writes profiles/reconstruct_ab.txt; --out FILE for another place, --out ""
                                          to print only)

The driver never touches the GPU.  Every measurement is a fresh worker process (this file with --worker loop|batch)
started under its own ``timeout``; --processes of each path, alternating; a worker warms up, then times --repeats whole
calls with a host clock around work that ends in a device synchronise, and prints their median.  The first worker
that fails, is killed by its time limit or dies of a signal ends the run: nothing more is started after it.  Reported
per path: the median over the processes' medians and their spread [min .. max], in ms per batch.

Synthetic shapes (synthetic.make_batch_ids), the labels as cluster ids, the deterministic SplineNets of the test
suite, epsilon 0.1.  No statement about the speed of either path holds before this file has been run on an MI355X
and its record committed."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def worker(a):
    import numpy as np
    import torch
    from parsenet_codebase_amd import metrics, synthetic
    from parsenet_codebase_amd.fitting import SIOU_matched_segments, to_one_hot
    from src.model import DGCNNControlPoints
    from src.residual_utils import Evaluation
    from src.segment_utils import sample_from_collection_of_mesh
    from tests.golden.common import deterministic_init
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    ids = [int(i) for i in a.ids.split(",")]
    pts, nrm, lab, prim = synthetic.make_batch_ids(ids, a.points, min_segments=4, max_segments=6)
    cid = np.stack([metrics.continuous_labels(x) for x in lab])
    ev = Evaluation(closed_path=deterministic_init(DGCNNControlPoints(20, num_points=10, mode=1), salt=1),
                    open_path=deterministic_init(DGCNNControlPoints(20, num_points=10, mode=0)))
    P, Nr = torch.from_numpy(pts).to(dev), torch.from_numpy(nrm).to(dev)
    seeds = [100 + i for i in ids]

    def loop():
        out = []
        for b in range(len(ids)):
            w = to_one_hot(cid[b], int(cid[b].max()) + 1, device_id=0)
            np.random.seed(seeds[b])
            with torch.no_grad():
                _, _, surfaces = ev.residual_eval_mode(P[b], Nr[b], lab[b], cid[b].copy(), prim[b], prim[b], w.T, 0.01,
                                                       sample_points=True, if_visualize=True, epsilon=0.1)
            m = metrics.coverage_metrics(torch.from_numpy(sample_from_collection_of_mesh(surfaces)).to(dev), P[b])
            m["s_iou"], m["p_iou"] = SIOU_matched_segments(lab[b], cid[b], prim[b], prim[b], w)[:2]
            out.append(m)
        return out

    def batch():
        return [r["metrics"] for r in ev.reconstruct_batch(P, Nr, lab, cid, prim, prim, seeds, epsilon=0.1)]

    fn = loop if a.worker == "loop" else batch
    times = []
    for r in range(a.warmup + a.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        if r >= a.warmup:
            times.append(1e3 * (time.perf_counter() - t0))
    times.sort()
    print("RESULT %s %.3f %.3f %.3f cd %s" % (a.worker, times[len(times) // 2], times[0], times[-1],
                                              " ".join("%.6e" % m["cd"] for m in res)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reconstruct_ab.txt"))
    ap.add_argument("--ids", default="3,11,21,40")
    ap.add_argument("--points", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="time limit of one worker process, seconds")
    ap.add_argument("--worker", choices=["loop", "batch"])
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("reconstruction metrics of shapes %s, %d points each; per path %d processes (alternating), each %d timed calls "
        "after %d warm-ups; whole call, ms per batch" % (a.ids, a.points, a.processes, a.repeats, a.warmup))
    medians = {"loop": [], "batch": []}
    ok = True
    for p in range(a.processes):
        for path in ("loop", "batch"):
            cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--worker", path,
                   "--ids", a.ids, "--points", str(a.points), "--repeats", str(a.repeats), "--warmup", str(a.warmup)]
            r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
            row = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")]
            if r.returncode != 0 or not row:
                say("process %d, %s: exit status %d — nothing more is started\n%s" % (p, path, r.returncode,
                                                                                       r.stderr[-2000:]))
                ok = False
                break
            f = row[0].split()
            medians[path].append(float(f[2]))
            say("process %d  %-5s median %9.3f  [%9.3f .. %9.3f]   %s" % (p, path, float(f[2]), float(f[3]), float(f[4]),
                                                                         " ".join(f[5:])))
        if not ok:
            break
    if ok:
        for path, label in (("loop", "(a) shape-by-shape loop"), ("batch", "(b) reconstruct_batch")):
            v = sorted(medians[path])
            say("%-26s median of the processes' medians %9.3f  [%9.3f .. %9.3f]" % (label, v[len(v) // 2], v[0], v[-1]))
        la, ba = sorted(medians["loop"]), sorted(medians["batch"])
        say("(a) / (b) = %.2f" % (la[len(la) // 2] / ba[len(ba) // 2]))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
