"""A/B of the LS refit's matchings at the refit's own sizes: (a) the host path — every distance matrix downloaded and
solved by scipy on the assignment pool — against (b) the device path — ONE auction launch over all matrices, costs
and prices downloaded, the exact finishes on the same pool.

    python tools/lsa_device_ab.py --out profiles/lsa_device_ab.txt

S = 16 matrices built by fitting_eval._refit_submit itself (its matching step is intercepted) from
synthetic.make_spline_patches: 8 open segments (1600 x 1600) and 8 closed ones (1600 x 2100); the "predicted"
control grids are the patches' own.  (b) is run over a grid of schedules (eps_final x theta); per schedule the
record has the auction's time (device events: warm-up, then repeats, median [min .. max]), its rounds, the number of
capped problems, the finish time (wall clock: download + pool) and whether every permutation equals (a)'s.  The
schedule and round cap in assignment.py are chosen from this record."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from parsenet_codebase_amd import _lsa_worker, assignment, fitting_eval, synthetic  # noqa: E402


def build_matrices(dev, per_kind):
    """The distance matrices of per_kind open and per_kind closed segments, as _refit_submit queues them."""
    taken = []
    orig = assignment.refit_submit
    assignment.refit_submit = lambda dist, host_submit: (taken.append(dist), (lambda: None))[1]
    try:
        for kind, closed in (("open", False), ("closed", True)):
            a_max = fitting_eval._RESAMPLE[kind][1]
            pts, ctrl = synthetic.make_spline_patches(40, per_kind, a_max, 20, closed=closed)
            P = torch.from_numpy(pts).to(dev)
            ctl = torch.from_numpy(ctrl).float().to(dev).reshape(per_kind, 20, 20, 3)
            affine = torch.eye(3, 4, device=dev).unsqueeze(0).repeat(per_kind, 1, 1).contiguous()
            rec = torch.zeros(per_kind, 900 if kind == "open" else 930, 3, device=dev)
            js = list(range(per_kind))
            draws = {j: {"refit": fitting_eval._refit_draws(kind, a_max)} for j in js}
            fitting_eval._refit_submit(kind, js, None, draws, P, ctl, affine, rec)
    finally:
        assignment.refit_submit = orig
    return taken


def stats(v):
    v = sorted(v)
    return "%9.2f [%9.2f .. %9.2f]" % (v[len(v) // 2], v[0], v[-1])


def pool_map(pool, fn, argss):
    if pool is None:
        return [fn(*a) for a in argss]
    return [j.result() for j in [pool.submit(fn, *a) for a in argss]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--per-kind", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--eps-final", type=float, nargs="*", default=[1e-3, 1e-4, 1e-5])
    ap.add_argument("--theta", type=float, nargs="*", default=[4.0, 6.0, 10.0])
    ap.add_argument("--max-rounds", type=int, default=assignment.MAX_ROUNDS)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    np.random.seed(3)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    mats = build_matrices(dev, a.per_kind)
    torch.cuda.synchronize()
    pool = fitting_eval.assignment_pool()
    say("LS refit matchings, S = %d: %s; pool of %s workers; %d repeats after one warm-up; ms, median [min .. max]"
        % (len(mats), ", ".join(sorted({"%d x %d" % tuple(m.shape) for m in mats})),
           "no" if pool is None else pool._max_workers, a.repeats))

    # (a) the host path: download, scipy on the raw matrices, side by side on the pool
    ref, t_a = None, []
    for r in range(a.repeats + 1):
        t0 = time.perf_counter()
        got = pool_map(pool, _lsa_worker.solve, [(m.cpu().numpy(),) for m in mats])
        if r:
            t_a.append((time.perf_counter() - t0) * 1e3)
        ref = got
    say("(a) host: download + scipy on the pool              %s" % stats(t_a))

    # (b) the device path per schedule
    say("(b) device: eps_start %g x range, round cap %d" % (assignment.EPS_START, a.max_rounds))
    say("    eps_final theta |            auction ms            | rounds median / max | capped |"
        "      download + finish ms        |             total ms             | permutations = (a)")
    best = None
    for ef in a.eps_final:
        for th in a.theta:
            kw = dict(eps_final=ef, theta=th, max_rounds=a.max_rounds)
            t_auc, t_fin, t_tot = [], [], []
            for r in range(a.repeats + 1):
                torch.cuda.synchronize()
                w0 = time.perf_counter()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                res = assignment.auction(mats, **kw)
                e1.record()
                e1.synchronize()
                w1 = time.perf_counter()
                prices = res["prices"].cpu().numpy()
                status = res["status"].cpu().numpy()
                jobs = [(assignment.finish_exact, (m.cpu().numpy(), prices[s, :m.shape[1]])) if status[s] == 0 else
                        (assignment.solve_host, (m.cpu().numpy(),)) for s, m in enumerate(mats)]
                if pool is None:
                    got = [fn(*args) for fn, args in jobs]
                else:
                    got = [j.result() for j in [pool.submit(fn, *args) for fn, args in jobs]]
                w2 = time.perf_counter()
                if r:
                    t_auc.append(e0.elapsed_time(e1))
                    t_fin.append((w2 - w1) * 1e3)
                    t_tot.append((w2 - w0) * 1e3)
            rounds = res["rounds"].cpu().numpy()
            same = all(np.array_equal(g, w) for g, w in zip(got, ref))
            capped = int((status != 0).sum())
            say("    %9.0e %5.1f | %s | %9d / %7d | %6d | %s | %s | %s"
                % (ef, th, stats(t_auc), int(np.median(rounds)), int(rounds.max()), capped, stats(t_fin), stats(t_tot),
                   "all equal" if same else "DIFFER"))
            tot = sorted(t_tot)[len(t_tot) // 2]
            if capped == 0 and same and (best is None or tot < best[0]):
                best = (tot, ef, th, int(rounds.max()))
    if best is not None:
        say("smallest auction + finish total with no capped problem: eps_final %g, theta %g (%.2f ms; most rounds of a "
            "problem %d); (a) / (b) = %.2f" % (best[1], best[2], best[0], best[3],
                                              sorted(t_a)[len(t_a) // 2] / best[0]))
    else:
        say("no schedule completed every problem with (a)'s permutations")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if pool is not None:
        pool.shutdown(wait=True)


if __name__ == "__main__":
    main()
