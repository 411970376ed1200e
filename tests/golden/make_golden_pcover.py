"""Generate tests/golden/pcover.npz by running the REFERENCE's own functions on the CPU:

    python tests/golden/make_golden_pcover.py

src.primitives.ResidualLoss(one_side=True, reduce=False).residual_loss(..., sqrt=True) is the reference's (imported
under the stubs of make_golden.py), once on float32 tensors and once on the same values as float64.  Only DATA is
written: points, primitive parameters, spline samples, the (S, N) distances of both runs, their minimum, the mean, the
cover at 0.01 and noise[type] = max |fp32 - fp64| per primitive type.  The tests take 4 x noise[type] as their bar.

Three synthetic shapes in the unit box, points drawn near the surfaces:
  a: 1 237 points (no multiple of 64 or 256); plane, sphere, cylinder, cone, an open spline of 900 samples, a closed
     spline of 930 samples, a second copy of the plane (the tie rule) and one None entry;
  b: 300 points, the two splines only;      c: 300 points, the four analytic primitives only.
The generator ABORTS when an input leaves the ground the tests stand on:
  * more than 1 % of a shape's points with a float64 minimum within the bar of 0.01 (excused from the cover comparison);
  * more than 2 % of a shape's points whose two smallest float64 distances, among primitives that are not bit-identical
    copies, lie within twice the bar (excused from the arg comparison);
  * a primitive that is nearest for no point.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests.golden.make_golden import install_stubs, save  # noqa: E402

TYPES = ["plane", "sphere", "cylinder", "cone", "open-spline", "closed-spline"]
SIGMA = 0.008     # noise of the points about their surface: most distances above guard_sqrt's floor of 3.2e-3


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def frame(a):
    h = np.array([1.0, 0, 0]) if abs(a[0]) < 0.9 else np.array([0, 1.0, 0])
    u = unit(np.cross(a, h))
    return u, np.cross(a, u)


def primitives():
    """name -> (entry data as float32 arrays, sampler(rng, n) of points on the surface)"""
    f32 = lambda *v: [np.asarray(x, np.float32) for x in v]   # noqa: E731
    out = {}
    a, d = unit([0.05, -0.03, 1.0]), -0.4
    u, v = frame(a)
    out["plane"] = (f32(a.reshape(3, 1), d),
                    lambda r, n: d * a + r.uniform(-0.45, 0.45, (n, 1)) * u + r.uniform(-0.45, 0.45, (n, 1)) * v)
    c, rad = np.array([-0.25, -0.25, 0.1]), 0.15

    def sphere(r, n):
        q = r.randn(n, 3)
        q[:, 2] = np.abs(q[:, 2])
        return c + rad * q / np.linalg.norm(q, axis=1, keepdims=True)
    out["sphere"] = (f32(c, rad), sphere)
    ax, cc, cr = unit([0.03, 0.02, 1.0]), np.array([0.27, -0.27, 0.0]), 0.1
    cu, cv = frame(ax)

    def cylinder(r, n):
        ang, h = r.uniform(0, 2 * np.pi, (n, 1)), r.uniform(-0.2, 0.4, (n, 1))
        return cc + h * ax + cr * (np.cos(ang) * cu + np.sin(ang) * cv)
    out["cylinder"] = (f32(ax.reshape(3, 1), cc, cr), cylinder)
    apex, ca, theta = np.array([0.25, 0.25, 0.45]), unit([0.02, -0.03, -1.0]), 0.3
    ku, kv = frame(ca)

    def cone(r, n):
        ang, h = r.uniform(0, 2 * np.pi, (n, 1)), r.uniform(0.15, 0.6, (n, 1))
        return apex + h * ca + h * np.tan(theta) * (np.cos(ang) * ku + np.sin(ang) * kv)
    out["cone"] = (f32(apex.reshape(1, 3), ca.reshape(3, 1), theta), cone)

    def open_surface(s, t):
        return np.stack([-0.25 + s, 0.25 + t, 0.2 + 0.8 * s * s - 0.6 * t * t + 0.2 * s], -1)
    s, t = np.meshgrid(np.linspace(-0.15, 0.15, 30), np.linspace(-0.15, 0.15, 30), indexing="ij")
    out["open-spline"] = (f32(open_surface(s, t).reshape(1, 900, 3)),
                          lambda r, n: open_surface(r.uniform(-0.15, 0.15, n), r.uniform(-0.15, 0.15, n)))

    def closed_surface(ang, h):
        rr = 0.05 + 0.015 * np.cos(12 * h)
        return np.stack([rr * np.cos(ang), rr * np.sin(ang), 0.3 + h], -1)
    ang = np.linspace(0, 2 * np.pi, 31)
    ang[-1] = 0.0
    g, hh = np.meshgrid(ang, np.linspace(-0.15, 0.15, 30), indexing="ij")
    out["closed-spline"] = (f32(closed_surface(g, hh).reshape(1, 930, 3)),
                            lambda r, n: closed_surface(r.uniform(0, 2 * np.pi, n), r.uniform(-0.15, 0.15, n)))
    return out


def reference_distances(residual_cls, points, entries, dtype):
    """(S, N) distances of the reference in ``dtype`` for the entries that are not None, in dict order"""
    prm = {k: (None if e is None else [e[0]] + [torch.from_numpy(x).to(dtype) for x in e[1]]) for k, e in entries.items()}
    for k, e in prm.items():
        if e is not None and e[0].endswith("spline"):
            prm[k] = [e[0], e[1]]                      # params[0][0] = the (M, 3) samples
    pts = torch.from_numpy(points).to(dtype)
    res = residual_cls(one_side=True, reduce=False).residual_loss({k: pts for k in prm}, prm, sqrt=True)
    return torch.stack([v[1] for v in res.values()], 0).numpy()


def main():
    install_stubs()
    from src.primitives import ResidualLoss
    prims = primitives()
    rng = np.random.RandomState(2025)
    shapes = {"a": (["plane", "sphere", "cylinder", "cone", "open-spline", "closed-spline", "plane", None], 1237),
              "b": (["open-spline", "closed-spline"], 300),
              "c": (["plane", "sphere", "cylinder", "cone"], 300)}
    arrays = {"types": np.asarray(TYPES)}
    for name in TYPES:
        for i, x in enumerate(prims[name][0]):
            arrays["%s_p%d" % (name, i)] = x
    noise = {t: 0.0 for t in TYPES}
    runs = {}
    for tag, (names, n) in shapes.items():
        live = [x for x in names if x is not None]
        distinct = sorted(set(live), key=live.index)
        owner = rng.randint(0, len(distinct), n)
        owner[:len(distinct)] = np.arange(len(distinct))
        pts = np.zeros((n, 3))
        for j, x in enumerate(distinct):
            m = owner == j
            pts[m] = prims[x][1](rng, int(m.sum()))
        pts = (pts + SIGMA * rng.randn(n, 3)).astype(np.float32)
        assert np.abs(pts).max() <= 0.5 + 6 * SIGMA
        entries = {k: (None if x is None else (x, prims[x][0])) for k, x in enumerate(names)}
        d32 = reference_distances(ResidualLoss, pts, entries, torch.float32)
        d64 = reference_distances(ResidualLoss, pts, entries, torch.float64)
        assert d32.dtype == np.float32 and d64.dtype == np.float64 and d32.shape == (len(live), n)
        for s, x in enumerate(live):
            noise[x] = max(noise[x], float(np.abs(d32[s].astype(np.float64) - d64[s]).max()))
        arrays.update({tag + "_points": pts, tag + "_names": np.asarray([x or "none" for x in names]),
                       tag + "_d32": d32, tag + "_d64": d64, tag + "_min32": d32.min(0),
                       tag + "_min64": d64.min(0), tag + "_mean32": np.asarray(torch.from_numpy(d32.min(0)).mean().item(), np.float32),
                       tag + "_cover32": np.asarray((d32.min(0) < 0.01).astype(np.float32).mean(), np.float32)})
        runs[tag] = (live, d64)
    arrays["noise"] = np.asarray([noise[t] for t in TYPES])
    for t in TYPES:
        print("noise %-14s %.3e -> bar %.3e" % (t, noise[t], 4 * noise[t]))
    bar = {t: 4 * noise[t] for t in TYPES}
    for tag, (live, d64) in runs.items():
        n = d64.shape[1]
        win = d64.argmin(0)
        wbar = np.asarray([bar[live[s]] for s in win])
        near_cover = np.abs(d64.min(0) - 0.01) <= wbar
        # the two smallest among primitives that are not bit-identical copies (later copies of an earlier row dropped)
        keep = np.asarray([s for s in range(len(live)) if live[s] not in live[:s]])
        sub, col = d64[keep], np.arange(n)
        order = sub.argsort(0)
        tbar = np.asarray([bar[live[s]] for s in keep])
        close = (sub[order[1], col] - sub[order[0], col] <= 2 * np.maximum(tbar[order[0]], tbar[order[1]])) \
            if len(keep) > 1 else np.zeros(n, bool)
        counts = np.bincount(keep[order[0]], minlength=len(live))
        print("shape %s: %4d points, %d primitives; nearest counts %s; %d near 0.01, %d near a tie; mean %.6f cover %.4f"
              % (tag, n, len(live), counts[keep].tolist(), near_cover.sum(), close.sum(),
                 float(arrays[tag + "_mean32"]), float(arrays[tag + "_cover32"])))
        assert near_cover.mean() <= 0.01, "shape %s: %.2f %% of the points within the bar of 0.01" % (tag, 100 * near_cover.mean())
        assert close.mean() <= 0.02, "shape %s: %.2f %% of the points near a tie" % (tag, 100 * close.mean())
        assert (counts[keep] > 0).all(), "shape %s: a primitive is nearest for no point" % tag
        arrays[tag + "_near_cover"] = near_cover
        arrays[tag + "_near_tie"] = close
    save("pcover", **arrays)


if __name__ == "__main__":
    main()
