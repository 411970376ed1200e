"""The EVALUATION-mode fitting stage, stage by stage over all shapes and segments of a batch.

What it computes is ``Evaluation.fitting_loss(eval=True)`` of the reference —
src/residual_utils.py:210-331 (residual_eval_mode: hard memberships, the modal PREDICTED primitive type
of every predicted segment, fits on the segment's own points, sqrt residuals), src/primitive_forward.py:
925-1047 (fit_one_shape_torch with eval=True), src/fitting_utils.py:704-710 (remove_outliers: open3d's
statistical outlier removal), :202-219 (up_sample_points_in_range: kNN-centroid up-sampling into the range
the SplineNets were trained on), src/primitive_forward.py:153-296 (the optional LS refit) — organised like
the training stage of fitting_batch.py instead of one segment after the other:

  clustering   bandwidths, mean-shift iterations, NMS and labels of all shapes as batched launches, ONE
               download of the cluster ids (fitting_batch's kernels; no autograd graph);
  host         Hungarian matching of every shape, the modal predicted type and the member lists of its
               segments, ONE packed upload;
  primitives   the four launches of csrc/fitbatch.hip for every analytic segment of the batch, with HARD
               one-hot membership rows (weight 1 + eps on the members, exactly 0 elsewhere, eps = 0 in the
               kernel: the moments of the members alone) and sqrt residuals;
  splines      outlier statistic of ALL spline segments from one ragged float64 neighbour search
               (csrc/knn3.hip, k = 20), ONE download of the surviving counts (they size numpy's draws);
               the up-sampling rounds as ragged float32 searches (k = 5) over the segments that still need
               one; ONE SplineNet forward per net over its re-sampled segments (all of one size), B-spline
               evaluation, the optional refit with its solves batched, ONE ragged Chamfer call.

numpy's generator is consumed in the reference's order — per shape: the shuffle of its mean-shift call(s),
then, segment by segment, the re-sampling draw and the draws of the refit — because every draw depends on
counts only, which the host has after the two downloads.  The per-segment functions of fitting.py
(``Evaluation.batched = False``) compute the same numbers one segment at a time; tests hold the two equal.

``fit_stage`` is everything after the clustering and starts from given cluster ids; ``reconstruct_batch`` (at the end
of the file) builds test.py's table of a set of shapes on it: trimmed surfaces, their samples, coverage and IoUs."""
import os

import numpy as np
import torch
from torch.profiler import record_function

from . import _lsa_worker
from . import assignment
from . import kernels as K
from . import mean_shift as MSM
from ._lib import h2d
from .fitting_batch import (CMAX, EPS, PRIM_CODE, _BSplineEval, _fitter_bases, bandwidth_batch, nms_batch,
                            standardize_segments)
from .kernels import KNN3_MAX_POINTS

_CLOSED_TYPES, _OPEN_TYPES = (0, 9, 6, 7), (2, 8)
_RESAMPLE = {"closed": (1400, 1800), "open": (1000, 1500)}      # src/primitive_forward.py:989-996, 1030-1036
_REFIT = {"open": dict(size_u=20, size_v=20, up=(1600, 2000), sub=1600, degree=2, bgrid=20),   # :229-296
          "closed": dict(size_u=21, size_v=20, up=(2000, 2100), sub=None, degree=3, bgrid=30)}  # :153-226


# ---------------------------------------------------------------------------------------------
# clustering of all shapes (no gradient)
# ---------------------------------------------------------------------------------------------
CALLS_CLUSTER = {"batched": 0, "per_shape": 0}      # shapes by the branch of cluster_shapes that clustered them


def cluster_shapes(ev, emb, quantile, iterations, kernel_type="gaussian"):
    """guard_mean_shift of every shape (src/residual_utils.py:69-84) -> (clusters, calls): clusters[b] =
    (centres (C,128), bandwidth (0-dim tensor), cluster ids (N,) int64 numpy), calls[b] = the number of
    mean-shift calls the guard needed for shape b.  The fast path is fitting_batch's: one batched bandwidth
    selection, the iterations of all shapes per launch, NMS and labels on the device, one download; a shape
    with flagged selection rows or more than 49 clusters goes through the per-shape API (the guard's retry
    with quantile x 1.2).  ``kernel_type``: the kernel of the iterations on both branches ("gaussian", or
    anything else for Epanechnikov); bandwidth, NMS and labels do not depend on it.

    numpy's generator is left where it was: the reference shuffles once per mean-shift call
    (src/mean_shift.py:121-122; every row is a sample, so the shuffle does not change the result) and the
    caller replays calls[b] shuffles at shape b's place in the stream."""
    B, N, D = emb.shape
    dev = emb.device
    fast = None
    with torch.no_grad():
        # every width up to 128 takes the batched branch at the width its kernels run at (fitting_batch._fitting_stage:
        # zero-padded once; zero columns are exact in every product); the centres are sliced back to D below
        W = MSM.kernel_width(D)
        embw = emb if W is None or W == D else torch.nn.functional.pad(emb, (0, W - D))
        bwres = bandwidth_batch(embw, quantile) if W is not None else None
        if bwres is not None:
            bw, bwflag = bwres
            MSM.WANT_NEAREST = True
            try:
                new_X, _ = MSM.mean_shift_iterations_state(embw, bw, iterations, kernel_type=kernel_type)
            finally:
                MSM.WANT_NEAREST = False
            nearest, MSM.LAST_NEAREST = MSM.LAST_NEAREST, None
            st = nms_batch(new_X, embw, bw, None, labels=True, nearest=nearest)
            if st is not None:
                pack = torch.cat([st["labels"].reshape(-1), st["cid"].reshape(-1), st["ncl"], bwflag,
                                  st["nflag"]]).to(torch.int32).cpu().numpy()              # download 1
                fast = (new_X, bw, pack[:B * N].reshape(B, N), pack[B * N:B * N + B * CMAX].reshape(B, CMAX),
                        pack[-3 * B:-2 * B], pack[-2 * B:-B], pack[-B:])
    clusters, calls = [], []
    state = np.random.get_state()
    for b in range(B):
        ok = fast is not None and fast[6][b] == 0 and fast[5][b] == 0 and fast[4][b] <= CMAX
        if ok and fast[4][b] <= 49:
            new_X, bw, lab_h, cid_h, ncl_h = fast[:5]
            cid = h2d(cid_h[b, :int(ncl_h[b])].astype(np.int64), dev)
            clusters.append((new_X[b][cid][:, :D], bw[b], lab_h[b].astype(np.int64)))
            calls.append(1)
            CALLS_CLUSTER["batched"] += 1
            continue
        # the guard's loop on the per-shape API; a fast attempt that found more than 49 clusters was its first call
        CALLS_CLUSTER["per_shape"] += 1
        q, n = (quantile * 1.2, 1) if ok else (quantile, 0)
        while True:
            _, center, bandwidth, ids = ev.ms.mean_shift(emb[b], 10000, q, iterations, kernel_type=kernel_type)
            n += 1
            if center.shape[0] > 49 and torch.unique(ids).shape[0] > 49:
                q *= 1.2
            else:
                break
        clusters.append((center, bandwidth.reshape(()), ids.cpu().numpy().astype(np.int64)))
        calls.append(n)
    np.random.set_state(state)
    return clusters, calls


# ---------------------------------------------------------------------------------------------
# host: matching and the segment list of one shape
# ---------------------------------------------------------------------------------------------
def eval_segments(labels, cluster_ids, pred_primitives, visualize=False):
    """residual_eval_mode's loop (src/residual_utils.py:233-262) + the dispatch rules of
    fit_one_shape_torch(eval=True): every matched predicted segment with its member indices, the indices of
    its ground-truth segment, the modal predicted type and the value of its hard membership column.
    ``visualize`` (the if_visualize rule, src/residual_utils.py:250-274): a predicted segment is kept even when its
    matched ground-truth segment is empty, and its own members stand in for the ground truth.
    Returns (segments in the reference's order, match (rows, cols, unique_target, unique_pred))."""
    from .fitting import match
    labels = np.asarray(labels)
    pred_primitives = np.asarray(pred_primitives)
    rows, cols, unique_target, unique_pred = match(labels, cluster_ids)
    width = np.unique(cluster_ids).shape[0]                 # columns of the one-hot membership matrix
    segs = []
    for index, i in enumerate(unique_pred):
        gt_idx = np.flatnonzero(labels == cols[index])
        pred_idx = np.flatnonzero(cluster_ids == i)
        if pred_idx.size == 0 or (gt_idx.size == 0 and not visualize):
            continue
        if visualize:
            gt_idx = pred_idx
        seg_type = int(np.bincount(pred_primitives[pred_idx].astype(np.int64)).argmax())
        kind = "closed" if seg_type in _CLOSED_TYPES else "open" if seg_type in _OPEN_TYPES else "prim"
        if kind == "prim" and seg_type not in PRIM_CODE:
            raise ValueError("unknown primitive type %r" % (seg_type,))
        # the segment reads column ``index`` of the one-hot of the cluster ids (src/primitive_forward.py:940):
        # 1 where the id equals that column
        wv = (1.0 if (int(i) == index and index < width) else 0.0) + EPS
        segs.append({"index": index, "key": int(i), "type": seg_type, "kind": kind, "pred": pred_idx, "gt": gt_idx,
                     "wv": np.float32(wv), "fit": pred_idx.size >= (20 if kind == "prim" else 100)})
    return segs, (rows, cols, unique_target, unique_pred)


# ---------------------------------------------------------------------------------------------
# ragged helpers
# ---------------------------------------------------------------------------------------------
def _ragged(counts, dev):
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return off, h2d(off, dev)


def outlier_keep_mask(pts, off_h, off_d):
    """remove_outliers (src/fitting_utils.py:704-710 -> open3d 0.9 remove_statistical_outlier(20, 0.5)) for a
    ragged batch of segments: pts (total,3) fp32, offsets on host and device.  Mean distance of every point to
    its 20 nearest neighbours (itself included) in float64, threshold = mean + 0.5 std (Bessel) over the
    segment, keep 0 < mean distance < threshold.  Returns the keep mask (total,) bool; the statistics of a
    segment are sums over its padded row in index order (no atomics)."""
    S = off_h.shape[0] - 1
    counts = np.diff(off_h)
    nmax = int(counts.max())
    k = int(min(20, counts.min()))
    if counts.min() < 20:       # a segment shorter than the neighbourhood: the search returns what there is (n)
        raise ValueError("outlier removal of a segment with fewer than 20 points")
    if nmax <= KNN3_MAX_POINTS:
        _, dist = K.knn3_ragged(pts, off_d, nmax, k, f64=True, want_dist=True)
    else:
        # a segment beyond the kernel's size (shapes of more than 10 240 points): float64 differences block-wise
        # and topk, segment by segment — what fitting._knn_points_by_differences and the reference fall back on
        dist = torch.cat([_mean_dist_broadcast(pts[off_h[s]:off_h[s + 1]].double(), k) for s in range(S)], 0)
    avg = dist.mean(1)                                                         # (total,) fp64
    dev = pts.device
    seg = torch.repeat_interleave(torch.arange(S, device=dev), h2d(counts.astype(np.int64), dev),
                                  output_size=int(off_h[-1]))
    pos = torch.arange(int(off_h[-1]), device=dev) - off_d[:-1].long()[seg]
    pad = torch.zeros((S, nmax), dtype=torch.float64, device=dev)
    valid = avg > 0
    n_t = h2d(counts.astype(np.float64), dev)
    pad[seg, pos] = torch.where(valid, avg, torch.zeros_like(avg))
    cloud_mean = pad.sum(1) / n_t
    dev2 = torch.zeros((S, nmax), dtype=torch.float64, device=dev)
    dev2[seg, pos] = torch.where(valid, (avg - cloud_mean[seg]) ** 2, torch.zeros_like(avg))
    std = torch.sqrt(dev2.sum(1) / torch.clamp(n_t - 1, min=1))
    std = torch.where(n_t > 1, std, torch.zeros_like(std))
    return valid & (avg < (cloud_mean + 0.5 * std)[seg])


def _mean_dist_broadcast(p, k):
    """(n,k) float64 distances of every point to its k nearest (itself included), 2 048 queries at a time."""
    out = []
    for s0 in range(0, p.shape[0], 2048):
        q = p[s0:s0 + 2048]
        dx, dy, dz = (q[:, None, c] - p[None, :, c] for c in range(3))
        d = (dx * dx + dy * dy) + dz * dz
        out.append(torch.sqrt(torch.topk(d, k, 1, largest=False)[0]))
    return torch.cat(out, 0)


def upsample_rounds(pts, counts, rounds):
    """up_sample_points_torch (src/fitting_utils.py:150-164) ``rounds[s]`` times on segment s of a ragged batch:
    each round appends the centroid of the 4 nearest neighbours of every point (csrc/knn3.hip, k = 5, fp32
    differences).  pts (total,3), counts / rounds host arrays.  Returns (pts, counts) after all rounds; a
    round runs over the segments that still need one."""
    dev = pts.device
    counts = np.asarray(counts, dtype=np.int64).copy()
    rounds = np.asarray(rounds, dtype=np.int64).copy()
    while rounds.max(initial=0) > 0:
        S = counts.shape[0]
        off = np.concatenate([[0], np.cumsum(counts)])
        act = np.flatnonzero(rounds > 0)
        # the active segments as a ragged batch of their own
        a_counts = counts[act]
        a_off_h, a_off_d = _ragged(a_counts, dev)
        src = np.concatenate([np.arange(off[s], off[s + 1]) for s in act])
        src_d = h2d(src, dev)
        sub = pts[src_d]
        idx = K.knn3_ragged(sub, a_off_d, int(a_counts.max()), 5)                 # local indices, self first
        seg = torch.repeat_interleave(torch.arange(act.shape[0], device=dev), h2d(a_counts, dev),
                                      output_size=int(a_off_h[-1]))
        glob = idx[:, 1:].long() + a_off_d[:-1].long()[seg].unsqueeze(1)
        centers = torch.mean(sub[glob], 1)
        # new layout: every active segment doubles to [points, centres]
        new_counts = counts.copy()
        new_counts[act] *= 2
        new_off = np.concatenate([[0], np.cumsum(new_counts)])
        dst_old = np.concatenate([np.arange(new_off[s], new_off[s] + counts[s]) for s in range(S)])
        dst_new = np.concatenate([np.arange(new_off[s] + counts[s], new_off[s + 1]) for s in act])
        out = torch.empty((int(new_off[-1]), 3), dtype=pts.dtype, device=dev)
        out[h2d(dst_old, dev)] = pts
        out[h2d(dst_new, dev)] = centers
        pts, counts = out, new_counts
        rounds[act] -= 1
    return pts, counts


def _rounds_to_reach(n, a_max):
    """up_sample_points(_torch)_in_range: at least one doubling, until n >= a_max."""
    if n <= 0:
        raise ValueError("up-sampling of an empty segment")
    r = 1
    while n * (1 << r) < a_max:
        r += 1
    return r


# ---------------------------------------------------------------------------------------------
# the stage
# ---------------------------------------------------------------------------------------------
class _Stream:
    """Where numpy's draws of the fitting stage come from.  The stage asks in the reference's order: ``begin(b)``
    before the first segment of shape b, ``analytic(b, segment)`` at every fitted analytic segment, ``end(b)`` after
    the last; the draws of the spline segments are taken from numpy's global generator in between."""

    def begin(self, b):
        pass

    def analytic(self, b, seg):
        pass

    def end(self, b):
        pass


class _ShuffleStream(_Stream):
    """fitting_loss(eval=True): the caller's stream, every shape preceded by the shuffle of its mean-shift call(s)."""

    def __init__(self, ms_calls, N):
        self.ms_calls, self.N = ms_calls, N

    def begin(self, b):
        for _ in range(self.ms_calls[b]):
            np.random.shuffle(np.arange(self.N))


def segment_draws(seglists, kept, if_optimize, stream):
    """numpy's draws of the fitting stage in the reference's order — shape by shape, segment by segment: for a
    spline segment the re-sampling draw and the draws of the refit (every draw depends on counts alone: ``kept[(b,
    key)]``, the points outlier removal left), for an analytic one whatever ``stream.analytic`` takes.  Host only.
    Returns {(b, key): draws of the spline segment}."""
    draws = {}
    for b, segs in enumerate(seglists):
        stream.begin(b)
        for s in segs:
            if not s["fit"]:
                continue
            if s["kind"] == "prim":
                stream.analytic(b, s)
                continue
            a_max = _RESAMPLE[s["kind"]][1]
            n = int(kept[(b, s["key"])])
            d = {}
            if n > a_max:
                d["rounds"] = 0
                d["L"] = np.random.choice(np.arange(n), a_max, replace=False)
            else:
                d["rounds"] = _rounds_to_reach(n, a_max)
                d["L"] = np.random.choice(np.arange(n << d["rounds"]), a_max, replace=False)
            if if_optimize and (s["kind"] == "open" or s["pred"].size > 200):
                d["refit"] = _refit_draws(s["kind"], a_max)
            draws[(b, s["key"])] = d
        stream.end(b)
    return draws


def fit_stage(ev, points, normals, seglists, ids_dev, if_optimize, stream, plane_means=False, net_batch=True):
    """Everything of the evaluation-mode fitting stage after the clustering, from GIVEN cluster ids: the primitive
    launches, the spline stage, the optional refit and the ONE download of distances, status and parameters.
    points / normals (B,N,3) fp32 on the device; seglists[b]: eval_segments of shape b; ids_dev (B,N) int64, the
    cluster ids on the device (-1: a padding row, member of no segment); ``stream``: see _Stream.
    ``plane_means``: also the mean of every plane segment's projected members (the expression of
    FittingModule.forward_pass_plane), in the same download.  ``net_batch=False``: standardisation, SplineNet and
    B-spline evaluation run segment by segment instead of once per net — the tensor library picks other GEMM kernels
    for other batch sizes (3e-5 in the samples), and a caller whose results must not depend on the batch a shape is
    evaluated in pays one forward per segment for that.  Call under torch.no_grad().
    Returns a dict: prim_segs / spl_segs (lists of (b, segment)), recs {j: (1, 900 | 930, 3) samples of spline j},
    dist_p / dist_s (device), dp / ds / pf / means (host, float64; means keyed by the position in prim_segs),
    params (device, fp32 rows), parameters[b] and fitted[b] (key -> ("prim" | "spline", position))."""
    B, N = points.shape[0], points.shape[1]
    dev = points.device
    fitter = ev.fitter
    prim_segs = [(b, s) for b in range(B) for s in seglists[b] if s["kind"] == "prim" and s["fit"]]
    spl_segs = [(b, s) for b in range(B) for s in seglists[b] if s["kind"] != "prim" and s["fit"]]
    flat_pts = points.reshape(B * N, 3)

    # ---- analytic primitives: hard membership rows, the members' moments --------------------------
    params = status = dist_p = pf = None
    means = []
    if prim_segs:
        Cp = max(sum(1 for bb, _ in prim_segs if bb == b) for b in range(B))
        row_of = {}
        seg_id = np.full((B, Cp), -2, np.int64)             # (-2: no segment; -1 marks padding rows of ids_dev)
        seg_wv = np.zeros((B, Cp), np.float32)
        nxt = [0] * B
        for b, s in prim_segs:
            row_of[(b, s["key"])] = nxt[b]
            seg_id[b, nxt[b]] = s["key"]
            seg_wv[b, nxt[b]] = s["wv"]
            nxt[b] += 1
        W = (ids_dev.unsqueeze(1) == h2d(seg_id, dev).unsqueeze(2)).float() * h2d(seg_wv, dev).unsqueeze(2)
        gt_lists = [s["gt"] for _, s in prim_segs]
        tab = {"shape": h2d(np.asarray([b for b, _ in prim_segs], np.int32), dev),
               "row": h2d(np.asarray([row_of[(b, s["key"])] for b, s in prim_segs], np.int32), dev),
               "type": h2d(np.asarray([PRIM_CODE[s["type"]] for _, s in prim_segs], np.int32), dev),
               "rows": h2d(np.asarray([s["pred"].size for _, s in prim_segs], np.int32), dev),
               "gt_off": h2d(np.concatenate([[0], np.cumsum([g.size for g in gt_lists])]).astype(np.int32), dev),
               "gt_idx": h2d(np.concatenate(gt_lists).astype(np.int32), dev)}
        with record_function("eval:primitives"):
            partial = K.weighted_moments(points, normals, W, tab["shape"], tab["row"], 1, 0.0)
            params, jac, status = K.primitive_fit(partial, tab["type"], tab["rows"])
            K.cone_angle(points, W, tab["shape"], tab["row"], tab["type"], status, params, jac, 1, 0.0)
            dist_p, _ = K.primitive_residual(points, tab["shape"], tab["type"], tab["gt_off"], tab["gt_idx"],
                                             params, status, True)
        pf = params.float()
        if plane_means:
            from .fitting import project_to_plane
            for k, (b, s) in enumerate(prim_segs):
                if PRIM_CODE[s["type"]] == K.PRIM_PLANE:
                    member = flat_pts[h2d(s["pred"] + b * N, dev)]
                    means.append((k, torch.mean(project_to_plane(member, pf[k, 0:3].reshape(1, 3), pf[k, 3]), 0)))

    # ---- splines -----------------------------------------------------------------------------------
    recs = {}
    dist_s = None
    kept = {}
    if spl_segs:
        members = np.concatenate([s["pred"] + b * N for b, s in spl_segs])
        counts0 = np.asarray([s["pred"].size for _, s in spl_segs], np.int64)
        seg_pts = flat_pts[h2d(members, dev)]
        off_h, off_d = _ragged(counts0, dev)
        with record_function("eval:outliers"):
            keep = outlier_keep_mask(seg_pts, off_h, off_d)
            csum = torch.cumsum(keep.long(), 0)
            ends = off_d[1:].long() - 1
            tot = csum[ends]
            kept_d = torch.cat([tot[:1], tot[1:] - tot[:-1]])
            kept_h = kept_d.cpu().numpy().astype(np.int64)                              # download 2
            if (kept_h < 5).any():
                # every mean distance equal (std 0: nothing is below the mean) or coincident points: the
                # reference's up-sampling raises in topk on such a cloud (src/fitting_utils.py:155-158) and
                # its caller skips the shape — never pad a segment with self-neighbours
                j = int(np.flatnonzero(kept_h < 5)[0])
                raise RuntimeError("fitting: outlier removal left %d point(s) of spline segment %d of shape %d "
                                   "(up-sampling needs 5)" % (kept_h[j], spl_segs[j][1]["key"], spl_segs[j][0]))
            seg_pts = seg_pts[keep]
        kept = {(b, s["key"]): kept_h[j] for j, (b, s) in enumerate(spl_segs)}
    # numpy's draws in the reference's order (every draw depends on counts alone, which the host now has)
    by_key = segment_draws(seglists, kept, if_optimize, stream)
    if spl_segs:
        draws = {j: by_key[(b, s["key"])] for j, (b, s) in enumerate(spl_segs)}
        with record_function("eval:upsample"):
            up_pts, up_counts = upsample_rounds(seg_pts, kept_h, [draws[j]["rounds"] for j in range(len(spl_segs))])
        up_off = np.concatenate([[0], np.cumsum(up_counts)])
        nu, nv = _fitter_bases(fitter, dev)
        groups = {"open": [j for j, (_, s) in enumerate(spl_segs) if s["kind"] == "open"],
                  "closed": [j for j, (_, s) in enumerate(spl_segs) if s["kind"] == "closed"]}
        pending_groups = []
        for kind, js in groups.items():
            if not js:
                continue
            a_max = _RESAMPLE[kind][1]
            sel = np.concatenate([up_off[j] + draws[j]["L"] for j in js])
            P = up_pts[h2d(sel, dev)].reshape(len(js), a_max, 3)
            w = h2d(np.asarray([spl_segs[j][1]["wv"] for j in js], np.float32), dev).reshape(-1, 1).expand(-1, a_max)
            w = w.contiguous()
            with record_function("eval:splinenet"):
                net = fitter.open_control_decoder if kind == "open" else fitter.closed_control_decoder
                parts = []
                for c in ([slice(0, len(js))] if net_batch else [slice(t, t + 1) for t in range(len(js))]):
                    pts_std, std, mean, R = standardize_segments(P[c], w[c])
                    aff = torch.cat([torch.linalg.inv(R) * std.unsqueeze(1), mean.unsqueeze(2)], 2).contiguous()
                    cp = net(K.transpose12(pts_std), w[c]).reshape(-1, 20, 20, 3)
                    parts.append((cp, aff, _BSplineEval.apply(cp, nu, nv, aff, kind == "closed")))  # (S,900|930,3)
                ctrl, affine, rec = (x[0] if len(parts) == 1 else torch.cat(x) for x in zip(*parts))
            # if_optimize: the refits of BOTH kinds are submitted (their matchings run on the assignment pool) before
            # either is finished
            pending_groups.append((js, _refit_submit(kind, js, spl_segs, draws, P, ctrl, affine, rec)
                                   if if_optimize else (lambda rec=rec: rec)))
        for js, fin in pending_groups:
            rec = fin()
            for t, j in enumerate(js):
                recs[j] = rec[t:t + 1]
        # two-sided Chamfer with guard_sqrt on every nearest-neighbour distance (src/utils.py:326-358)
        order = list(range(len(spl_segs)))
        pred = torch.cat([recs[j].reshape(-1, 3) for j in order], 0)
        na = [int(recs[j].shape[1]) for j in order]
        nb = [spl_segs[j][1]["gt"].size for j in order]
        gt_cloud = flat_pts[h2d(np.concatenate([spl_segs[j][1]["gt"] + spl_segs[j][0] * N for j in order]), dev)]
        off_a = h2d(np.concatenate([[0], np.cumsum(na)]).astype(np.int32), dev)
        off_b = h2d(np.concatenate([[0], np.cumsum(nb)]).astype(np.int32), dev)
        with record_function("eval:chamfer"):
            minA, _, minB, _ = K.chamfer_nn_ragged(pred, off_a, max(na), gt_cloud, off_b, max(nb))
            gs = lambda x: torch.sqrt(torch.clamp(x, min=1e-5))                       # noqa: E731
            dist_s = K.chamfer_ragged_reduce(gs(minA), off_a, gs(minB), off_b)

    # ---- ONE download of the distances (and the fit status), then the per-shape records -------------
    tail = []
    if prim_segs:
        tail += [dist_p.double(), status.double(), params.reshape(-1)]
        if means:
            tail.append(torch.stack([m for _, m in means]).double().reshape(-1))
    if spl_segs:
        tail.append(dist_s.double())
    host = torch.cat(tail).cpu().numpy() if tail else np.zeros(0)                      # download 3
    o = 0
    Sp, Ss = len(prim_segs), len(spl_segs)
    dp_h = pf_h = None
    means_h = {}
    if prim_segs:
        dp_h, st_h = host[:Sp], host[Sp:2 * Sp].astype(np.int64)
        pf_h = host[2 * Sp:2 * Sp + Sp * params.shape[1]].reshape(Sp, -1)
        o = 2 * Sp + pf_h.size
        if (st_h & 5).any():
            bad = int(np.nonzero(st_h & 5)[0][0])
            raise RuntimeError("fitting: %s in segment %d of shape %d" % (
                "non-finite design matrix / no full-rank ridge system (lstsq)" if st_h[bad] & 1 else
                "NaN residual distance", prim_segs[bad][1]["key"], prim_segs[bad][0]))
        for t, (k, _) in enumerate(means):
            means_h[k] = host[o + 3 * t:o + 3 * t + 3]
        o += 3 * len(means)
    ds_h = host[o:o + Ss]
    parameters, fitted_all = [], []
    for b in range(B):
        prm, fitted = {}, {}
        for k, (bb, s) in enumerate(prim_segs):
            if bb == b:
                fitted[s["key"]] = ("prim", k)
        for j, (bb, s) in enumerate(spl_segs):
            if bb == b:
                fitted[s["key"]] = ("spline", j)
        for s in seglists[b]:
            if s["key"] not in fitted:
                prm[s["key"]] = None
                continue
            what, k = fitted[s["key"]]
            if what == "prim":
                code, p = PRIM_CODE[s["type"]], pf[k]
                if code == K.PRIM_PLANE:
                    prm[s["key"]] = ["plane", p[0:3].reshape(3, 1), p[3]]
                elif code == K.PRIM_SPHERE:
                    prm[s["key"]] = ["sphere", p[0:3].reshape(1, 3), p[3]]
                elif code == K.PRIM_CYLINDER:
                    prm[s["key"]] = ["cylinder", p[0:3].reshape(3, 1), p[3:6].reshape(1, 3), p[6]]
                else:
                    prm[s["key"]] = ["cone", p[0:3].reshape(1, 3), p[3:6].reshape(3, 1), p[6:7]]
                d = float(dp_h[k])
            else:
                prm[s["key"]] = ["open-spline" if s["kind"] == "open" else "closed-spline", recs[k]]
                d = float(ds_h[k])
            if not np.isfinite(d):
                raise RuntimeError("fitting: non-finite residual distance in segment %d of shape %d" % (s["key"], b))
        parameters.append(prm)
        fitted_all.append(fitted)
    return {"prim_segs": prim_segs, "spl_segs": spl_segs, "recs": recs, "dist_p": dist_p, "dist_s": dist_s,
            "dp": dp_h, "ds": ds_h, "pf": pf_h, "means": means_h, "params": pf, "parameters": parameters,
            "fitted": fitted_all, "downloads": (1 if tail else 0) + (1 if spl_segs else 0)}


def fitting_losses_eval(ev, embedding, points, normals, labels, primitives, primitives_log_prob, quantile, iterations,
                        lamb, if_optimize=False, kernel_type="gaussian"):
    """Evaluation-mode Evaluation.fitting_loss for every shape of the batch: a list (one entry per shape) of
    ([Loss, geometric mean, spline mean, s_iou, p_iou], [parameters, cluster ids, weights]) as the reference's
    call with that single shape returns them.  ``kernel_type``: the kernel of the clustering (cluster_shapes)."""
    from .fitting import SIOU_matched_segments, to_one_hot
    B, N, D = embedding.shape
    dev = embedding.device
    labels, primitives = np.asarray(labels), np.asarray(primitives)
    points, normals = points.contiguous().float(), normals.contiguous().float()
    with torch.no_grad():
        emb = torch.nn.functional.normalize(embedding.detach(), p=2, dim=2)
        prim_pred = torch.max(primitives_log_prob, 1)[1].data.cpu().numpy()
        with record_function("eval:clustering"):
            clusters, ms_calls = cluster_shapes(ev, emb, quantile, iterations, kernel_type=kernel_type)
        seglists = [eval_segments(labels[b], clusters[b][2], prim_pred[b])[0] for b in range(B)]
        ids_dev = h2d(np.stack([c[2] for c in clusters]).astype(np.int64), dev)           # (B,N)
        st = fit_stage(ev, points, normals, seglists, ids_dev, if_optimize, _ShuffleStream(ms_calls, N))
        dp_h, ds_h, dist_p, dist_s = st["dp"], st["ds"], st["dist_p"], st["dist_s"]
        out = []
        for b in range(B):
            parameters, fitted = st["parameters"][b], st["fitted"][b]
            geo, spl, loss_terms = [], [], []
            # separate_losses (src/residual_utils.py:333-378): in ascending key order
            for key in sorted(k_ for k_, v in parameters.items() if v is not None):
                what, k = fitted[key]
                d = float(dp_h[k]) if what == "prim" else float(ds_h[k])
                dt = dist_p[k] if what == "prim" else dist_s[k]
                if d > 1:                               # most probably a degenerate case
                    d, dt = 0.1, torch.ones((), device=dev) * 0.1
                if what == "prim":
                    geo.append(float(d))
                    loss_terms.append(dt)
                else:
                    spl.append(float(d))
                    loss_terms.append(dt * lamb)
            Loss = torch.mean(torch.stack(loss_terms)) if loss_terms else torch.zeros(1, device=dev)
            ids_b = clusters[b][2]
            weights = to_one_hot(ids_b, np.unique(ids_b).shape[0], device_id=dev.index).T
            s_iou, p_iou, _, _ = SIOU_matched_segments(labels[b], ids_b, prim_pred[b], primitives[b], weights.T)
            out.append(([Loss, np.mean(geo) if geo else None, np.mean(spl) if spl else None, s_iou, p_iou],
                        [parameters, ids_b, weights]))
    return out


def _refit_draws(kind, a_max):
    """numpy's draws of one optimize_*_spline_kronecker call (src/primitive_forward.py:153-296), in its order:
    the uniform (u, v) parameters, the re-sampling of the up-sampled input points, the sub-sample."""
    from .fitting import boundary_parameterization
    cfg = _REFIT[kind]
    nbound = boundary_parameterization(cfg["bgrid"]).shape[0]
    d = {"uv": np.random.random((1600 - nbound, 2))}
    lo, hi = cfg["up"]
    n = a_max
    if n > hi:
        d["rounds"] = 0
        d["L"] = np.random.choice(np.arange(n), hi, replace=False)
    else:
        d["rounds"] = _rounds_to_reach(n, hi)
        d["L"] = np.random.choice(np.arange(n << d["rounds"]), hi, replace=False)
    if cfg["sub"] is not None:
        d["sub"] = np.random.choice(np.arange(hi), cfg["sub"], replace=False)
    return d


# ---------------------------------------------------------------------------------------------
# assignment pool: the Hungarian matchings of a batch's refits side by side
# ---------------------------------------------------------------------------------------------
_LSA_POOL = None
# matchings of the LS refit by the path that solved them (PARSENET_REFIT_LSA = host | device; "capped": the device
# auction hit its round cap and the problem went to the host solver)
CALLS_LSA = assignment.CALLS_LSA
REFIT_POOL = os.environ.get("PARSENET_REFIT_POOL", "1") != "0"


def assignment_pool():
    """A persistent pool of worker PROCESSES (spawned: they import numpy / scipy only, never torch) for the
    linear_sum_assignment calls of the LS refit — scipy holds the GIL, threads would run them one after the other.
    Sized by the CPUs the job may use (dp.usable_cpus() - 1, at most 16).  None when PARSENET_REFIT_POOL=0 or a single CPU:
    the caller then solves in place."""
    global _LSA_POOL
    if not REFIT_POOL:
        return None
    if _LSA_POOL is None:
        import atexit
        import multiprocessing
        from concurrent.futures import ProcessPoolExecutor
        from .dp import usable_cpus
        n = min(16, usable_cpus() - 1)      # (a batch of 4 shapes has up to 16 spline segments: one matching per worker)
        if n < 2:
            return None
        _LSA_POOL = ProcessPoolExecutor(max_workers=n, mp_context=multiprocessing.get_context("spawn"))
        atexit.register(_LSA_POOL.shutdown, wait=False, cancel_futures=True)
    return _LSA_POOL


def _refit_batch(kind, js, spl_segs, draws, P, ctrl, affine, rec):
    """The LS refit of one kind in one go (submit, then finish)."""
    return _refit_submit(kind, js, spl_segs, draws, P, ctrl, affine, rec)()


def _refit_submit(kind, js, spl_segs, draws, P, ctrl, affine, rec):
    """The LS refit (src/primitive_forward.py:153-296) of the segments ``js`` of one kind: samples of the
    predicted surface at the drawn parameters, the input points up-sampled (ragged, together) and re-sampled,
    the Hungarian matching per segment on the host (scipy), the 100 x 100 normal equations of all segments
    solved together, the refitted surfaces sampled on the regular grid.  Segments the reference does not refit
    (closed, 200 members or fewer) keep their network prediction.

    Two phases (round 6): this function queues everything up to the distance matrices and hands them to the
    assignment pool; the returned ``finish()`` collects the matchings and runs the solves.  The caller submits BOTH
    kinds of a batch before it finishes either, so all matchings of the batch run side by side on the host's cores
    (14.1 s -> see profiles/r06_named_kernels_kbench.txt per batch of 4 shapes, all of it scipy's assignment)."""
    from .approximation import fit_bezier_surface_fit_kronecker
    from .bspline import basis_matrix, uniform_knots
    from .fitting import boundary_parameterization, regular_parameterization, solve_dense
    cfg = _REFIT[kind]
    dev = P.device
    todo = [t for t, j in enumerate(js) if "refit" in draws[j]]
    if not todo:
        return lambda: rec
    S = len(todo)
    a_max = P.shape[1]
    su, sv = cfg["size_u"], cfg["size_v"]
    # control grid in the input frame; closed: the first row appended again (21 x 20)
    grid = ctrl[todo]
    if kind == "closed":
        grid = torch.cat([grid, grid[:, 0:1]], 1)
    aff = affine[todo]
    grid = grid.reshape(S, su * sv, 3) @ aff[:, :, :3].transpose(1, 2) + aff[:, :, 3].unsqueeze(1)
    bound = boundary_parameterization(cfg["bgrid"])
    ku, kv = uniform_knots(su, 3), uniform_knots(sv, 3)
    ku2 = uniform_knots(10, cfg["degree"])
    reg = regular_parameterization(30, 30)
    RU = torch.from_numpy(basis_matrix(reg[:, 0], 10, cfg["degree"], ku2)).to(dev)
    RV = torch.from_numpy(basis_matrix(reg[:, 1], 10, cfg["degree"], ku2)).to(dev)
    # input points of all segments up-sampled together
    rounds = [draws[js[t]]["refit"]["rounds"] for t in todo]
    up, cnt = upsample_rounds(P[todo].reshape(S * a_max, 3), [a_max] * S, rounds)
    off = np.concatenate([[0], np.cumsum(cnt)])
    out = rec.clone()
    pool = assignment_pool()

    def host_submit(cost):
        if pool is not None:
            return pool.submit(_lsa_worker.solve, cost).result
        return lambda: solve_dense(cost)[1]
    pending = []
    for q, t in enumerate(todo):
        d = draws[js[t]]["refit"]
        parameters = np.concatenate([d["uv"], bound], 0)
        bu = torch.from_numpy(basis_matrix(parameters[:, 0], su, 3, ku)).to(dev)
        bv = torch.from_numpy(basis_matrix(parameters[:, 1], sv, 3, kv)).to(dev)
        samples = torch.einsum("ni,nj,ijc->nc", bu, bv, grid[q].reshape(su, sv, 3).double())      # (1600,3) fp64
        inp = up[h2d(off[q] + d["L"], dev)]
        if "sub" in d:
            inp = inp[h2d(d["sub"], dev)]
        inp = inp.double()
        dist = torch.cdist(samples, inp, compute_mode="donot_use_mm_for_euclid_dist")
        # PARSENET_REFIT_LSA=device: the matrix stays on the GPU and joins the batch's ONE auction launch, which the
        # first finish() of either kind triggers (assignment.queue_device)
        pending.append((t, parameters, inp, assignment.refit_submit(dist, host_submit)))

    def finish():
        for t, parameters, inp, matching in pending:
            cids = matching()
            matched = inp[h2d(np.asarray(cids), dev)]
            NU = torch.from_numpy(basis_matrix(parameters[:, 0], 10, cfg["degree"], ku2)).to(dev)
            NV = torch.from_numpy(basis_matrix(parameters[:, 1], 10, cfg["degree"], ku2)).to(dev)
            new_ctrl = fit_bezier_surface_fit_kronecker(matched, NU, NV)
            pts = torch.einsum("ni,nj,ijc->nc", RU, RV, new_ctrl).float()
            if kind == "closed":
                pts = pts.reshape(30, 30, 3)
                pts = torch.cat([pts, pts[0:1]], 0).reshape(930, 3)
            out[t] = pts
        return out
    return finish


# ---------------------------------------------------------------------------------------------
# reconstruction metrics of a batch of shapes (test.py:108-185), from GIVEN cluster ids
# ---------------------------------------------------------------------------------------------
# shapes served; grid_occupancy calls (one per batch that has a surface); device -> host transfers issued by
# reconstruct_batch and the fitting stage under it (SIOU_matched_segments' type vote, one per shape, and the
# matchings of the refit are not counted)
CALLS_RECONSTRUCT = {"shapes": 0, "occupancy_launches": 0, "downloads": 0}


class ShapeStreams(_Stream):
    """The random-number contract of reconstruct_batch: shape b consumes numpy's stream as if np.random.seed(seeds[b])
    had been called just before it — per segment, in the reference's order, the re-sampling and refit draws of a
    spline and the two draws of sample_plane, then the draws of sample_from_collection_of_mesh.  The fitting-stage
    draws of ALL shapes come first (they depend on counts only); the state of every shape's generator after them is
    kept (``sampler_state``), and so is the state in front of every plane's two draws (``plane_state``: sample_plane
    takes them itself once the fitted parameters are on the host).  ``sampler_draws`` continues shape b from its saved
    state.  Use through ``shape_streams``, which restores the caller's global state."""

    def __init__(self, seeds):
        self.seeds = [int(s) for s in seeds]
        self.plane_state, self.sampler_state = {}, {}

    def begin(self, b):
        np.random.seed(self.seeds[b])

    def analytic(self, b, seg):
        if PRIM_CODE[seg["type"]] == K.PRIM_PLANE:
            self.plane_state[(b, seg["key"])] = np.random.get_state()
            np.random.random()
            np.random.random()

    def end(self, b):
        self.sampler_state[b] = np.random.get_state()

    def sample_plane(self, b, key, d, n, mean):
        from .surface import sample_plane
        np.random.set_state(self.plane_state[(b, key)])
        return sample_plane(d, n, mean)

    def sampler_draws(self, b, counts):
        from .surface import sample_draws
        np.random.set_state(self.sampler_state[b])
        draws = sample_draws(counts)
        self.sampler_state[b] = np.random.get_state()
        return draws


class shape_streams:
    """with shape_streams(seeds) as stream: ...  — numpy's global state is the caller's again afterwards."""

    def __init__(self, seeds):
        self.stream = ShapeStreams(seeds)

    def __enter__(self):
        self.state = np.random.get_state()
        return self.stream

    def __exit__(self, *exc):
        np.random.set_state(self.state)
        return False


def _reconstruct_args(points, normals, labels, cluster_ids, primitives, pred_primitives, seeds):
    """Argument checks of reconstruct_batch (host only) -> per-shape lists; ValueError names the shape."""
    def rows(x, name):
        if torch.is_tensor(x) or isinstance(x, np.ndarray):
            if x.ndim != 3 or x.shape[2] != 3:
                raise ValueError("reconstruct_batch: %s must be (B,N,3) or a list of (N_b,3), got %s"
                                 % (name, tuple(x.shape)))
            return [x[b] for b in range(x.shape[0])], True
        return list(x), False
    pts, whole = rows(points, "points")
    nrm, _ = rows(normals, "normals")
    B = len(pts)
    if B < 1:
        raise ValueError("reconstruct_batch: no shape")
    seeds = np.asarray(seeds).reshape(-1)
    if seeds.shape[0] != B:
        raise ValueError("reconstruct_batch: %d seeds for %d shapes (shape %d has none)"
                         % (seeds.shape[0], B, min(seeds.shape[0], B - 1)))
    ints = {}
    for name, x in (("normals", nrm), ("labels", labels), ("cluster_ids", cluster_ids), ("primitives", primitives),
                    ("pred_primitives", pred_primitives)):
        if len(x) != B:
            raise ValueError("reconstruct_batch: %s of %d shapes, points of %d (shape %d)"
                             % (name, len(x), B, min(len(x), B - 1)))
        if name != "normals":
            ints[name] = [np.asarray(v.detach().cpu() if torch.is_tensor(v) else v).reshape(-1) for v in x]
    for b in range(B):
        n = pts[b].shape[0] if pts[b].ndim else 0
        if pts[b].ndim != 2 or pts[b].shape[1] != 3 or n < 1:
            raise ValueError("reconstruct_batch: shape %d: points must be (N,3) with N >= 1, got %s"
                             % (b, tuple(pts[b].shape)))
        if tuple(nrm[b].shape) != (n, 3):
            raise ValueError("reconstruct_batch: shape %d: %d points, normals %s" % (b, n, tuple(nrm[b].shape)))
        for name, v in ints.items():
            if v[b].shape[0] != n:
                raise ValueError("reconstruct_batch: shape %d: %d points, %d %s" % (b, n, v[b].shape[0], name))
        # the one-hot encodings of the metrics scatter by these values: keep them inside their widths
        cid = ints["cluster_ids"][b]
        if cid.min() < 0 or np.unique(cid).shape[0] != int(cid.max()) + 1:
            raise ValueError("reconstruct_batch: shape %d: cluster ids must be 0..K-1 without gaps "
                             "(metrics.continuous_labels relabels them)" % b)
        for name in ("primitives", "pred_primitives"):
            if ints[name][b].min() < 0 or ints[name][b].max() > 9:
                raise ValueError("reconstruct_batch: shape %d: %s outside 0..9" % (b, name))
    return (pts, nrm, ints["labels"], ints["cluster_ids"], ints["primitives"], ints["pred_primitives"],
            [int(s) for s in seeds], whole)


def _device_rows(rows, whole, given, dev):
    """(B,Nmax,3) fp32 on the device from per-shape rows (zero rows pad the shorter shapes)."""
    if whole and torch.is_tensor(given):
        return given.detach().to(dev).float().contiguous()
    rows = [r.detach().to(dev).float() if torch.is_tensor(r) else h2d(np.asarray(r, np.float32), dev) for r in rows]
    nmax = max(r.shape[0] for r in rows)
    return torch.stack([torch.nn.functional.pad(r, (0, 0, 0, nmax - r.shape[0])) for r in rows]).contiguous()


def reconstruct_batch(ev, points, normals, labels, cluster_ids, primitives, pred_primitives, seeds, bw=0.01,
                      if_optimize=False, if_visualize=True, epsilon=None, n_samples=10000, surface_distance=False,
                      kernel_type="gaussian"):
    """What test.py:108-185 computes for one shape — residual_eval_mode(sample_points=True), the trimmed surfaces,
    sample_from_collection_of_mesh, the coverage figures and the IoUs — for B shapes, stage by stage: the fitting
    stage of this module from the GIVEN cluster ids (no embedding, no mean-shift), the analytic grids on the host in
    float64 (surface.sample_*), ONE occupancy call and one mask download for all segments of all shapes, one area and
    one sampling launch for all surfaces, one ragged Chamfer call and one coverage reduction (csrc/chamfer.hip) whose
    (B,6) table is all the metrics download.  ``if_optimize`` gives the trimmed surfaces of the LS refit (its sample
    grids), which the per-segment entry does not provide.

    points / normals: (B,N,3) or lists of (N_b,3), arrays or tensors; labels, cluster_ids, primitives,
    pred_primitives: integer arrays per shape; seeds: one integer per shape (the random-number contract:
    ShapeStreams; a batch equals the shape-by-shape loop under the same seeds, the caller's global state is restored).
    ``bw`` is accepted for the reference's signature: hard memberships do not depend on it.  ``kernel_type`` (last)
    is the kernel the given cluster ids were made with (cluster_shapes): a caller hands one set of clustering
    arguments to both; nothing after the clustering depends on the kernel profile.
    Returns one dict per shape: parameters (as residual_eval_mode), surfaces ([TrimmedSurface]), samples ((M_b,3) fp32
    on the device), metrics (sk_1, sk_2, sk, pk_1, pk_2, pk, cd, s_iou, p_iou) — or metrics None, samples None and
    ``message`` when the sampling of that shape fails (no surface with a kept cell, or none that gets more than 10
    points), as test.py:152-156 skips such a shape.  Argument errors raise ValueError with the shape index.
    ``surface_distance``: the metrics also carry p_cover_surface and p_dist_surface, sk_1 and sk taken against the
    trimmed surfaces themselves instead of their samples (metrics.surface_coverage_batch: two more launches and one
    more download for the batch; no random draw, nothing else changes)."""
    from . import surface
    from .fitting import SIOU_matched_segments, to_one_hot, up_sample_points_torch_memory_efficient
    from .metrics import coverage_rows, surface_coverage_batch
    pts_l, nrm_l, lab_l, cid_l, prim_l, pp_l, seeds, whole = _reconstruct_args(
        points, normals, labels, cluster_ids, primitives, pred_primitives, seeds)
    B = len(pts_l)
    seglists = []
    for b in range(B):
        try:
            seglists.append(eval_segments(lab_l[b], cid_l[b], pp_l[b], visualize=if_visualize)[0])
        except ValueError as e:
            raise ValueError("reconstruct_batch: shape %d: %s" % (b, e))
    dev = torch.device("cuda", torch.cuda.current_device())
    counts_n = [p.shape[0] for p in pts_l]
    downloads = 0
    with torch.no_grad(), shape_streams(seeds) as stream:
        P = _device_rows(pts_l, whole, points, dev)
        Nr = _device_rows(nrm_l, whole, normals, dev)
        N = P.shape[1]
        ids = np.full((B, N), -1, np.int64)
        for b in range(B):
            ids[b, :counts_n[b]] = cid_l[b]
        # (net_batch=False: a shape's spline grids — and with them its masks, samples and figures — are those of the
        # shape-by-shape loop whatever else is in the batch)
        st = fit_stage(ev, P, Nr, seglists, h2d(ids, dev), if_optimize, stream, plane_means=True, net_batch=False)
        downloads += st["downloads"]
        host_pts = None

        def members(b, s):
            nonlocal host_pts, downloads
            if host_pts is None:
                if any(torch.is_tensor(p) for p in pts_l):
                    host_pts = P.cpu().numpy()                                     # the batch's points, once
                    downloads += 1
                else:
                    host_pts = [np.asarray(p, np.float32) for p in pts_l]
            return host_pts[b][s["pred"]]

        # ---- grids: the stage's samples for splines, float64 on the host for analytic surfaces --------------
        entries = []                     # (b, segment, size, device grid | None, host grid | None)
        pf32 = None if st["pf"] is None else st["pf"].astype(np.float32)
        for b in range(B):
            for s in seglists[b]:
                what = st["fitted"][b].get(s["key"])
                if what is None:
                    continue
                rounds, eps_default, size = surface._TRIM[s["type"]]
                if what[0] == "spline":
                    entries.append([b, s, size, st["recs"][what[1]][0].float(), None])
                    continue
                k = what[1]
                p = pf32[k]
                code = PRIM_CODE[s["type"]]
                if code == K.PRIM_PLANE:
                    g = stream.sample_plane(b, s["key"], float(p[3]), p[0:3].reshape(1, 3),
                                            st["means"][k].astype(np.float32))
                elif code == K.PRIM_SPHERE:
                    g = surface.sample_sphere(float(p[3]), p[0:3].reshape(1, 3))
                elif code == K.PRIM_CYLINDER:
                    g = surface.sample_cylinder_trim(float(p[6]), p[3:6].copy(), p[0:3].copy(), members(b, s))
                else:
                    g = surface.sample_cone_trim(p[0:3].copy(), p[3:6].copy(), float(p[6]), members(b, s))
                g = np.asarray(g).astype(np.float32).reshape(-1, 3)
                if size is None:
                    size = (g.shape[0] // 51, 51)
                if size[0] < 2 or g.shape[0] != size[0] * size[1]:
                    continue        # (a cone whose trimming left fewer than two rings: nothing to tessellate)
                entries.append([b, s, size, None, g])
        analytic = [e for e in entries if e[3] is None]
        if analytic:
            up = h2d(np.concatenate([e[4] for e in analytic]), dev)               # one upload
            o = 0
            for e in analytic:
                e[3] = up[o:o + e[4].shape[0]]
                o += e[4].shape[0]
        # ---- occupancy: every segment of every shape in ONE call, one download ------------------------------
        surfaces = [[] for _ in range(B)]
        if entries:
            clouds = [up_sample_points_torch_memory_efficient(P[b][h2d(s["pred"], dev)], surface._TRIM[s["type"]][0])
                      for b, s, _, _, _ in entries]
            thres = [epsilon if epsilon else surface._TRIM[s["type"]][1] for _, s, _, _, _ in entries]
            masks = surface.grid_occupancy([e[3] for e in entries], [e[2] for e in entries], clouds, thres)
            CALLS_RECONSTRUCT["occupancy_launches"] += 1
            spl = [e for e in entries if e[4] is None]
            pack = torch.cat([e[3].reshape(-1) for e in spl] + [m.reshape(-1).float() for m in masks]).cpu().numpy()
            downloads += 1
            o = 0
            for e in spl:
                n = e[2][0] * e[2][1] * 3
                e[4] = pack[o:o + n].reshape(-1, 3)
                o += n
            for (b, s, (u, v), _, gh) in entries:
                n = (u - 1) * (v - 1)
                surfaces[b].append(surface.TrimmedSurface(gh, u, v, pack[o:o + n] != 0))
                o += n
        # ---- samples: one area launch, one sampling launch ---------------------------------------------------
        message = [None] * B
        meshes = [[m for m in surfaces[b] if m.mask.any()] for b in range(B)]
        for b in range(B):
            if not meshes[b]:
                message[b] = "sample_from_collection_of_mesh: no surface with a kept cell"
        flat = [m for b in range(B) for m in meshes[b]]
        sampled, counts, cdf, draws, shape_off = [], [], [], [], [0]
        if flat:
            # (own storage per surface: the order in which torch.sum adds depends on the alignment of the slice, and
            # a shape's figures must not depend on the batch it was evaluated in)
            areas = [a.clone() for a in surface.triangle_areas(flat, dev)]
            A = torch.stack([a.sum() for a in areas]).cpu().numpy()
            downloads += 1
            o = 0
            for b in range(B):
                nb = len(meshes[b])
                if nb:
                    cnt = surface.sample_counts(A[o:o + nb], n_samples)
                    take = [i for i, k in enumerate(cnt) if k > 0]
                    if not take:
                        message[b] = ("sample_from_collection_of_mesh: no surface gets more than 10 of the %d points"
                                      % n_samples)
                    else:
                        draws += stream.sampler_draws(b, [cnt[i] for i in take])
                        for i in take:
                            a = areas[o + i]
                            a = a + torch.min(a) + 1e-10
                            c = torch.cumsum(a / torch.sum(a), 0)
                            cdf.append(c / c[-1])
                            sampled.append(meshes[b][i])
                            counts.append(cnt[i])
                o += nb
                shape_off.append(int(np.sum(counts)))
        else:
            shape_off += [0] * B
        samples = [None] * B
        if sampled:
            grid, voff, sv, foff, cells, _ = surface._mesh_tables(sampled, dev)
            total = shape_off[-1]
            samp_off = np.concatenate([[0], np.cumsum(counts)])
            uni = h2d(np.concatenate([np.concatenate([d[j] for d in draws]) for j in range(3)]), dev)
            cdf_d = torch.cat(cdf).contiguous()
            out = torch.empty(total, 3, dtype=torch.float32, device=dev)
            from . import _lib
            with _lib.on_device(dev):
                rc = _lib.load().pn_trimesh_sample_f64(
                    _lib.ptr(grid), _lib.ptr(voff), _lib.ptr(sv), _lib.ptr(foff), _lib.ptr(cells), _lib.ptr(cdf_d),
                    _lib.ptr(h2d(samp_off.astype(np.int32), dev)), _lib.ptr(uni[:total]),
                    _lib.ptr(uni[total:2 * total]), _lib.ptr(uni[2 * total:]), len(sampled), total, _lib.ptr(out),
                    None, _lib.current_stream(dev))
            _lib.check(rc, "pn_trimesh_sample_f64")
            for b in range(B):
                if message[b] is None:
                    samples[b] = out[shape_off[b]:shape_off[b + 1]].clone()
        # ---- coverage: one ragged nearest-neighbour call, one reduction, one (S,6) download -------------------
        live = [b for b in range(B) if samples[b] is not None]
        rows = coverage_rows([samples[b] for b in live], [P[b, :counts_n[b]] for b in live]) if live else []
        downloads += 1 if live else 0
        exact = []
        if surface_distance and live:
            exact = surface_coverage_batch([P[b, :counts_n[b]] for b in live], [surfaces[b] for b in live])
            downloads += 1
        records = []
        for b in range(B):
            rec = {"parameters": st["parameters"][b], "surfaces": surfaces[b], "samples": samples[b], "metrics": None,
                   "message": message[b]}
            if samples[b] is not None:
                m = rows[live.index(b)]
                weights = to_one_hot(cid_l[b], np.unique(cid_l[b]).shape[0], device_id=dev.index)
                m["s_iou"], m["p_iou"], _, _ = SIOU_matched_segments(lab_l[b], cid_l[b], pp_l[b], prim_l[b], weights)
                if exact:
                    m.update(exact[live.index(b)])
                rec["metrics"] = m
            records.append(rec)
    CALLS_RECONSTRUCT["shapes"] += B
    CALLS_RECONSTRUCT["downloads"] += downloads
    return records
