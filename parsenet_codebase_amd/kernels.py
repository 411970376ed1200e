"""Tensor-level wrappers over the C ABI.  Each function validates layout, allocates
outputs/workspace through torch's caching allocator and launches on torch's current
HIP stream.  No arithmetic happens here."""
import math
import numbers

import numpy as np
import torch

from . import _lib
from ._lib import check, current_stream, ptr, require_cuda
from .ragged import Clouds


def _f32c(t, name):
    if t.dtype != torch.float32:
        raise TypeError("%s must be float32, got %s" % (name, t.dtype))
    return t.contiguous()


def chamfer_nn(a, b, side_a=True, side_b=True):
    """Nearest neighbours between two batched clouds.

    a: (B, Na, 3), b: (B, Nb, 3) fp32 on the GPU.
    Returns (minA, argA, minB, argB): for every a_i the squared distance to and index of
    its nearest b_j (ties -> smallest j), and vice versa.  Entries of a side that was not
    requested are None.
    """
    require_cuda(a, b)
    a = _f32c(a, "a")
    b = _f32c(b, "b")
    if a.dim() != 3 or b.dim() != 3 or a.shape[2] != 3 or b.shape[2] != 3 or a.shape[0] != b.shape[0]:
        raise ValueError("chamfer_nn expects (B,Na,3) and (B,Nb,3), got %s and %s"
                         % (tuple(a.shape), tuple(b.shape)))
    B, Na, _ = a.shape
    Nb = b.shape[1]
    if Na == 0 or Nb == 0 or B == 0:
        raise ValueError("chamfer_nn: empty cloud")
    lib = _lib.load()
    dev = a.device
    minA = argA = minB = argB = None
    if side_a:
        minA = torch.empty((B, Na), dtype=torch.float32, device=dev)
        argA = torch.empty((B, Na), dtype=torch.int64, device=dev)
    if side_b:
        minB = torch.empty((B, Nb), dtype=torch.float32, device=dev)
        argB = torch.empty((B, Nb), dtype=torch.int64, device=dev)
    wsz = lib.pn_chamfer_nn_workspace(B, Na, Nb)
    ws = torch.empty(wsz, dtype=torch.uint8, device=dev)
    with _lib.on_device(dev):
        rc = lib.pn_chamfer_nn_f32(ptr(a), ptr(b), B, Na, Nb, ptr(minA), ptr(argA), ptr(minB),
                                   ptr(argB), ptr(ws), wsz, current_stream(dev))
    check(rc, "pn_chamfer_nn_f32")
    return minA, argA, minB, argB


def knn(x, k, metric="feature", int32=False):
    """k nearest neighbours in feature space, self included, best first.

    x: (B, C, N) fp32 channel-first (the layout the reference's encoders use).
    metric: "feature" (src/model.py:9-22, src/PointNet.py:9-26) or "points_normals"
    (src/PointNet.py:29-69, C must be 6).  Returns idx (B, N, k) int64 — the dtype of the reference's
    ``topk`` indices — or, with ``int32``, the same values as int32: the form the library's edge-conv
    kernels take (half the index bytes), which the encoders use between their own layers.
    """
    require_cuda(x)
    x = _f32c(x, "x")
    if x.dim() != 3:
        raise ValueError("knn expects (B,C,N), got %s" % (tuple(x.shape),))
    if metric not in ("feature", "points_normals"):
        raise ValueError("unknown metric %r" % (metric,))
    B, C, N = x.shape
    if metric == "points_normals" and C != 6:
        raise ValueError("points_normals metric needs 6 channels, got %d" % C)
    lib = _lib.load()
    dev = x.device
    idx = torch.empty((B, N, k), dtype=torch.int32 if int32 else torch.int64, device=dev)
    wsz = lib.pn_knn_workspace(B, C, N, k)
    ws = torch.empty(wsz, dtype=torch.uint8, device=dev)
    with _lib.on_device(dev):
        if int32:
            rc = lib.pn_knn_graph_i32(ptr(x), B, C, N, k, int(metric == "points_normals"), ptr(idx), ptr(ws), wsz,
                                      current_stream(dev))
        elif metric == "feature":
            rc = lib.pn_knn_f32(ptr(x), B, C, N, k, ptr(idx), ptr(ws), wsz, current_stream(dev))
        else:
            rc = lib.pn_knn_pn_f32(ptr(x), B, N, k, ptr(idx), ptr(ws), wsz, current_stream(dev))
    check(rc, "pn_knn")
    return idx


KNN3_MAX_POINTS = 10240      # pn_knn3_ragged's limit on the points of one segment in fp32 mode: 160 values per lane


# The offsets of a ragged batch.  Every wrapper below takes ``off`` in the form it has always taken — a device int32
# tensor with ``max_n`` beside it (knn3_ragged, knn3_grid, fps_ragged), or host integers (point_normals and the two
# orient wrappers) — or the ``ragged.Clouds`` the points were flattened by: its host offsets serve the checks, its
# device offsets, uploaded once for all the kernels of a call, the launch, and ``max_n`` may be None.
# The device copy is asked for only where a kernel is launched: a call that returns early or refuses its arguments
# copies nothing, as before.
def _device_offsets(who, pts, off, max_n):
    """What knn3_ragged, knn3_grid and fps_ragged share -> (pts (total,3) fp32 contiguous, upload, S, max_n);
    ``upload()`` gives the offsets on the device as contiguous int32."""
    clouds = isinstance(off, Clouds)
    require_cuda(pts, None if clouds else off)
    pts = _f32c(pts, "pts")
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise ValueError("%s expects (total,3) points, got %s" % (who, tuple(pts.shape),))
    if clouds:
        if pts.shape[0] != off.total or pts.device != off.flat.device:
            raise ValueError("%s: pts %s on %s is not the flat array of the Clouds given as off (%d points on %s)"
                             % (who, tuple(pts.shape), pts.device, off.total, off.flat.device))
        return pts, off.device_offsets, off.S, off.max_n if max_n is None else int(max_n)
    if off.dtype != torch.int32:
        raise TypeError("off must be int32")
    return pts, off.contiguous, off.numel() - 1, int(max_n)


def _host_view(who, off):
    """The first thing point_normals and the two orient wrappers do with ``off`` -> (the offsets on the host, the
    Clouds they came in or None).  A device tensor is a TypeError."""
    if isinstance(off, Clouds):
        return off.off, off
    if torch.is_tensor(off):
        if off.is_cuda:
            raise TypeError("%s: off must be host integers (a list, an array or a CPU tensor)" % who)
        off = off.numpy()
    return off, None


def _host_offsets(who, off, total, k):
    """The check of the host offsets the same three share (ascending from 0 to total, row * k within int32)
    -> (offsets int64, S)."""
    off = np.asarray(off, np.int64).reshape(-1)
    S = off.shape[0] - 1
    if S < 0 or off[0] != 0 or off[-1] != total or (np.diff(off) < 0).any():
        raise ValueError("%s: off must ascend from 0 to %d" % (who, total))
    if total * max(k, 3) >= 2 ** 31:
        raise ValueError("%s: int32 offsets" % who)
    return off, S


def _upload_offsets(off, clouds, dev):
    """The offsets on ``dev`` as int32: the tensor the Clouds holds, or one stream-ordered copy of host integers."""
    return clouds.device_offsets() if clouds is not None else _lib.h2d(off.astype(np.int32), dev)


def knn3_ragged(pts, off, max_n, k, f64=False, want_dist=False):
    """Neighbours of 3-D points by coordinate differences inside the segments of a ragged batch
    (csrc/knn3.hip; src/fitting_utils.py:150-164, 704-710).  pts (total,3) fp32, off (S+1) int32 device
    offsets, max_n >= the largest segment (a host integer) — or off a ``ragged.Clouds`` and max_n None.  Returns idx
    (total,k) int32 LOCAL to the segment — nearest first, the point itself first — and, with ``want_dist``, their
    distances (float64 when ``f64``)."""
    pts, off, S, max_n = _device_offsets("knn3_ragged", pts, off, max_n)
    total = pts.shape[0]
    idx = torch.empty((total, k), dtype=torch.int32, device=pts.device)
    dist = torch.empty((total, k), dtype=torch.float64 if f64 else torch.float32, device=pts.device) if want_dist else None
    if total == 0 or S <= 0:
        return (idx, dist) if want_dist else idx
    with _lib.on_device(pts.device):
        rc = _lib.load().pn_knn3_ragged(ptr(pts), ptr(off()), S, max_n, int(k), int(bool(f64)), ptr(idx), ptr(dist),
                                        current_stream(pts.device))
    check(rc, "pn_knn3_ragged")
    return (idx, dist) if want_dist else idx


def knn3_grid(pts, off, max_n, k, want_dist=False):
    """``knn3_ragged``'s fp32 neighbours, bit for bit, by a uniform-grid search (csrc/knn3_grid.hip, definition
    csrc/knn3_grid_math.h): cost O(n k) and no limit on the size of a segment.  pts (total,3) fp32, off (S+1) int32
    device offsets, max_n >= the largest segment (a host integer) — or off a ``ragged.Clouds`` and max_n None.  Returns
    idx (total,k) int32 LOCAL to the segment — nearest first, the point itself first, equal distances to the smaller
    index, a segment shorter than k padded with the point itself — and, with ``want_dist``, their fp32 distances.
    1 <= k <= 64, total * k < 2^31.  A segment that holds a non-finite coordinate gets the point itself k times and NaN
    distances.  Five stream-ordered launches on a workspace linear in total, no host synchronisation."""
    pts, off, S, max_n = _device_offsets("knn3_grid", pts, off, max_n)
    k = int(k)
    total = pts.shape[0]
    if total * max(k, 1) >= 2 ** 31:
        raise ValueError("knn3_grid: total * k = %d (below 2^31)" % (total * k))
    idx = torch.empty((total, k), dtype=torch.int32, device=pts.device)
    dist = torch.empty((total, k), dtype=torch.float32, device=pts.device) if want_dist else None
    if total == 0 or S <= 0:
        return (idx, dist) if want_dist else idx
    lib = _lib.load()
    wsz = lib.pn_knn3_grid_workspace_bytes(total, S)
    ws = torch.empty(wsz, dtype=torch.uint8, device=pts.device)
    with _lib.on_device(pts.device):
        rc = lib.pn_knn3_grid_f32(ptr(pts), ptr(off()), S, total, max_n, k, ptr(idx), ptr(dist), ptr(ws), wsz,
                                  current_stream(pts.device))
    check(rc, "pn_knn3_grid_f32")
    return (idx, dist) if want_dist else idx


QUERY_MIN_K, QUERY_MAX_K = 1, 64


def _cloud_offsets(who, rows, off, what, dev):
    """The offsets of one ragged batch of ``rows`` rows on ``dev`` -> (upload, S).  ``off`` is a device int32 tensor or
    the ``ragged.Clouds`` the rows were flattened by."""
    if isinstance(off, Clouds):
        if rows != off.total or dev != off.flat.device:
            raise ValueError("%s: %d rows on %s do not belong to the Clouds given as %s (%d points on %s)"
                             % (who, rows, dev, what, off.total, off.flat.device))
        return off.device_offsets, off.S
    require_cuda(off)
    if off.dtype != torch.int32:
        raise TypeError("%s: %s must be int32" % (who, what))
    return off.contiguous, off.numel() - 1


def _pair_offsets(who, ref_rows, off_r, qry_rows, off_q, dev):
    """The offsets of a (reference, query) pair of ragged batches -> (upload_r, upload_q, S).  Each of off_r, off_q is
    a device int32 tensor or the ``ragged.Clouds`` its rows were flattened by; both must describe S clouds."""
    up_r, S_r = _cloud_offsets(who, ref_rows, off_r, "off_r", dev)
    up_q, S_q = _cloud_offsets(who, qry_rows, off_q, "off_q", dev)
    if S_r != S_q:
        raise ValueError("%s: off_r describes %d clouds, off_q %d" % (who, S_r, S_q))
    return up_r, up_q, max(S_r, 0)


def _query_k(who, k, rows):
    k = int(k)
    if not QUERY_MIN_K <= k <= QUERY_MAX_K:
        raise ValueError("%s: k must be %d .. %d, got %d" % (who, QUERY_MIN_K, QUERY_MAX_K, k))
    if rows * k >= 2 ** 31:
        raise ValueError("%s: totalQ * k = %d (below 2^31)" % (who, rows * k))
    return k


def knn3_query(ref, off_r, qry, off_q, k, want_dist=False):
    """The k nearest REFERENCE points of every query point, segment s of the queries searched in segment s of the
    reference (csrc/knn3_query.hip; grid, cells and bound of csrc/knn3_grid_math.h, built on the reference): exact, cost
    O((n_r + n_q) k), any sizes.  ref (totalR,3), qry (totalQ,3) fp32; off_r, off_q (S+1) int32 device offsets or the
    ``ragged.Clouds`` the points were flattened by.  Returns idx (totalQ,k) int32 LOCAL to the reference segment — the k
    smallest under the fp32 ((dx² + dy²) + dz²), equal distances to the smaller index — and, with ``want_dist``, their
    fp32 distances.  A reference of n_r < k points: idx -1 and dist +inf from entry n_r on.  A non-finite coordinate in
    the reference segment (every row of its queries) or in the query (that row): idx -1, dist NaN.  1 <= k <= 64,
    totalQ * k < 2^31.  ``pn_knn3_query_launches()`` = 8 stream-ordered launches on a workspace linear in both totals,
    no host synchronisation; the same bits from run to run and for every batching."""
    require_cuda(ref, qry)
    ref, qry = _f32c(ref, "ref"), _f32c(qry, "qry")
    for t, what in ((ref, "reference"), (qry, "query")):
        if t.dim() != 2 or t.shape[1] != 3:
            raise ValueError("knn3_query expects (total,3) %s points, got %s" % (what, tuple(t.shape)))
    if ref.device != qry.device:
        raise ValueError("knn3_query: the reference is on %s, the queries on %s" % (ref.device, qry.device))
    totalR, totalQ, dev = ref.shape[0], qry.shape[0], qry.device
    k = _query_k("knn3_query", k, totalQ)
    up_r, up_q, S = _pair_offsets("knn3_query", totalR, off_r, totalQ, off_q, dev)
    idx = torch.empty((totalQ, k), dtype=torch.int32, device=dev)
    dist = torch.empty((totalQ, k), dtype=torch.float32, device=dev) if want_dist else None
    if totalQ > 0 and S > 0:
        lib = _lib.load()
        wsz = lib.pn_knn3_query_workspace_bytes(totalR, totalQ, S)
        ws = torch.empty(wsz, dtype=torch.uint8, device=dev)
        with _lib.on_device(dev):
            rc = lib.pn_knn3_query_f32(ptr(ref), ptr(up_r()), totalR, ptr(qry), ptr(up_q()), totalQ, S, k, ptr(idx),
                                       ptr(dist), ptr(ws), wsz, current_stream(dev))
        check(rc, "pn_knn3_query_f32")
    return (idx, dist) if want_dist else idx


def _lift_args(who, off_r, totalR, idx, off_q):
    require_cuda(idx)
    idx = _i32c(idx, "idx")
    if idx.dim() != 2:
        raise ValueError("%s expects (totalQ,k) idx, got %s" % (who, tuple(idx.shape)))
    totalQ, k = idx.shape
    k = _query_k(who, k, totalQ)
    up_r, up_q, S = _pair_offsets(who, totalR, off_r, totalQ, off_q, idx.device)
    return idx, totalQ, k, up_r, up_q, S


def knn_interpolate(values, off_r, idx, dist, off_q):
    """Inverse-distance interpolation of per-reference-point values at the queries (csrc/knn_lift.hip, definition
    csrc/knn_lift_math.h; PointNet++'s three_interpolate for any k): values (totalR,C) fp32, idx and dist (totalQ,k) as
    ``knn3_query`` returned them for the same offsets.  out (totalQ,C) fp32 = (float)(Σ w_j v_j / Σ w_j),
    w_j = 1 / ((double) dist_j + 1e-8), in fp64 in ascending rank over the entries with idx >= 0.  A row with no such
    entry or with a NaN distance is NaN.  One launch, no host synchronisation."""
    require_cuda(values, dist)
    values, dist = _f32c(values, "values"), _f32c(dist, "dist")
    if values.dim() != 2 or values.shape[1] < 1:
        raise ValueError("knn_interpolate expects (totalR,C) values with C >= 1, got %s" % (tuple(values.shape),))
    totalR, C = values.shape
    idx, totalQ, k, up_r, up_q, S = _lift_args("knn_interpolate", off_r, totalR, idx, off_q)
    if dist.shape != idx.shape or dist.device != idx.device or values.device != idx.device:
        raise ValueError("knn_interpolate: dist %s must have the shape of idx %s, on the device of idx and values"
                         % (tuple(dist.shape), tuple(idx.shape)))
    if totalQ * C >= 2 ** 39:
        raise ValueError("knn_interpolate: totalQ * C = %d (below 2^39)" % (totalQ * C))
    out = torch.empty((totalQ, C), dtype=torch.float32, device=idx.device)
    if totalQ > 0 and S > 0:
        with _lib.on_device(idx.device):
            rc = _lib.load().pn_knn_interpolate_f32(ptr(values), ptr(up_r()), totalR, ptr(idx), ptr(dist), ptr(up_q()),
                                                    totalQ, S, k, C, ptr(out), current_stream(idx.device))
        check(rc, "pn_knn_interpolate_f32")
    return out


def knn_vote(labels, off_r, idx, off_q):
    """Majority vote of per-reference-point labels at the queries (csrc/knn_lift.hip, definition csrc/knn_lift_math.h):
    labels (totalR) int32, idx (totalQ,k) as ``knn3_query`` returned it for the same offsets.  out (totalQ) int32: the
    label >= 0 that occurs most often among the entries with idx >= 0, on equal counts the one with the nearer member;
    none: -1.  One launch, no host synchronisation."""
    require_cuda(labels)
    labels = _i32c(labels, "labels")
    if labels.dim() != 1:
        raise ValueError("knn_vote expects (totalR) labels, got %s" % (tuple(labels.shape),))
    totalR = labels.shape[0]
    idx, totalQ, k, up_r, up_q, S = _lift_args("knn_vote", off_r, totalR, idx, off_q)
    if labels.device != idx.device:
        raise ValueError("knn_vote: labels on %s, idx on %s" % (labels.device, idx.device))
    out = torch.empty(totalQ, dtype=torch.int32, device=idx.device)
    if totalQ > 0 and S > 0:
        with _lib.on_device(idx.device):
            rc = _lib.load().pn_knn_vote_i32(ptr(labels), ptr(up_r()), totalR, ptr(idx), ptr(up_q()), totalQ, S, k,
                                             ptr(out), current_stream(idx.device))
        check(rc, "pn_knn_vote_i32")
    return out


REGISTER_POINT, REGISTER_PLANE = 0, 1
REGISTER_MAX_ITER = 256


def _nonneg(who, name, v, allow_inf=False):
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or not v >= 0 or (math.isinf(v) and not allow_inf):
        raise ValueError("%s: %s must be a number >= 0%s, got %r" % (who, name, " (inf allowed)" if allow_inf else "", v))
    return float(v)


def _rows3(who, t, what):
    t = _f32c(t, what)
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError("%s expects (total,3) %s, got %s" % (who, what, tuple(t.shape)))
    return t


def _transforms(who, T, S, dev, name="transform"):
    """(S,16) fp64 contiguous on ``dev`` from a (S,4,4) or (S,16) float64 device tensor."""
    if not torch.is_tensor(T) or T.dtype != torch.float64:
        raise TypeError("%s: %s must be a float64 tensor" % (who, name))
    if T.numel() != 16 * S or T.dim() not in (2, 3):
        raise ValueError("%s: %s must be (%d,4,4), got %s" % (who, name, S, tuple(T.shape)))
    if T.device != dev:
        raise ValueError("%s: %s is on %s, the points on %s" % (who, name, T.device, dev))
    return T.reshape(S, 16).contiguous()


def register_ragged(src, off_s, tgt, off_t, max_dist, mode=REGISTER_POINT, normals=None, init=None, max_iter=50,
                    tol_rot=1e-6, tol_trans=1e-6, want_pairs=False):
    """Rigid registration of segment s of ``src`` (it moves) onto segment s of ``tgt`` by iterative closest point on the
    exact grid search of ``knn3_query`` (csrc/register.hip, definition csrc/register_math.h).  src (totalS,3), tgt
    (totalT,3), normals (totalT,3) or None, fp32; off_s, off_t (S+1) int32 device offsets or the ``ragged.Clouds`` the
    points were flattened by; init (S,4,4) float64 on the device or None (the identity).  mode REGISTER_POINT or
    REGISTER_PLANE (needs normals).  Returns transform (S,4,4) float64, iterations, status, count (S) int32, rmse (S)
    float64 and, with ``want_pairs``, idx (totalS) int32 and dist (totalS) fp32 of the final pairing.
    ``pn_register_launches(max_iter)`` = 12 + 9 max_iter stream-ordered launches, no host synchronisation; the same
    bits from run to run and for every batching."""
    who = "register_ragged"
    require_cuda(src, tgt, normals)
    src, tgt = _rows3(who, src, "source points"), _rows3(who, tgt, "target points")
    if mode not in (REGISTER_POINT, REGISTER_PLANE):
        raise ValueError("%s: mode must be REGISTER_POINT or REGISTER_PLANE, got %r" % (who, mode))
    if mode == REGISTER_PLANE and normals is None:
        raise ValueError("%s: REGISTER_PLANE needs the target's normals" % who)
    if normals is not None:
        normals = _rows3(who, normals, "normals")
        if normals.shape != tgt.shape or normals.device != tgt.device:
            raise ValueError("%s: normals %s must have the shape and the device of the target %s"
                             % (who, tuple(normals.shape), tuple(tgt.shape)))
    if src.device != tgt.device:
        raise ValueError("%s: the source is on %s, the target on %s" % (who, src.device, tgt.device))
    max_dist = _nonneg(who, "max_dist", max_dist, allow_inf=True)
    tol_rot, tol_trans = _nonneg(who, "tol_rot", tol_rot), _nonneg(who, "tol_trans", tol_trans)
    if isinstance(max_iter, bool) or not isinstance(max_iter, numbers.Integral) or not 1 <= max_iter <= REGISTER_MAX_ITER:
        raise ValueError("%s: max_iter must be an integer 1 .. %d, got %r" % (who, REGISTER_MAX_ITER, max_iter))
    totalS, totalT, dev = src.shape[0], tgt.shape[0], src.device
    up_t, up_s, S = _pair_offsets(who, totalT, off_t, totalS, off_s, dev)
    if init is not None:
        init = _transforms(who, init, S, dev, "init")
    T = torch.empty((S, 4, 4), dtype=torch.float64, device=dev)
    its, status, count = (torch.empty(S, dtype=torch.int32, device=dev) for _ in range(3))
    rmse = torch.empty(S, dtype=torch.float64, device=dev)
    idx = torch.empty(totalS, dtype=torch.int32, device=dev) if want_pairs else None
    dist = torch.empty(totalS, dtype=torch.float32, device=dev) if want_pairs else None
    if S > 0:
        lib = _lib.load()
        wsz = lib.pn_register_workspace_bytes(totalS, totalT, S)
        ws = torch.empty(wsz, dtype=torch.uint8, device=dev)
        with _lib.on_device(dev):
            rc = lib.pn_register_f32(ptr(src), ptr(up_s()), totalS, ptr(tgt), ptr(up_t()), totalT,
                                     ptr(normals) if mode == REGISTER_PLANE else None, S, int(mode), max_dist,
                                     int(max_iter), tol_rot, tol_trans, ptr(init), ptr(T), ptr(its), ptr(status),
                                     ptr(count), ptr(rmse), ptr(idx), ptr(dist), ptr(ws), wsz, current_stream(dev))
        check(rc, "pn_register_f32")
    out = (T, its, status, count, rmse)
    return out + (idx, dist) if want_pairs else out


def rigid_apply(src, off_s, transform):
    """The move step of the registration as a call of its own, the same bits (csrc/register.hip): src (totalS,3) fp32,
    off_s (S+1) int32 device offsets or a ``ragged.Clouds``, transform (S,4,4) float64 on the device.  Returns
    (totalS,3) fp32: (float)(((R00 x + R01 y) + R02 z) + t0) ... in fp64, R derived from the unit quaternion of the
    transform's rotation block.  One launch, no host synchronisation."""
    who = "rigid_apply"
    require_cuda(src)
    src = _rows3(who, src, "points")
    totalS, dev = src.shape[0], src.device
    up_s, S = _cloud_offsets(who, totalS, off_s, "off_s", dev)
    S = max(S, 0)
    T = _transforms(who, transform, S, dev)
    out = torch.empty_like(src)
    if S > 0 and totalS > 0:
        with _lib.on_device(dev):
            rc = _lib.load().pn_rigid_apply_f32(ptr(src), ptr(up_s()), S, totalS, ptr(T), ptr(out), current_stream(dev))
        check(rc, "pn_rigid_apply_f32")
    return out


NORMALS_MIN_K, NORMALS_MAX_K = 3, 64


def point_normals(pts, off, idx, k, viewpoints=None, want_scalars=False):
    """k-NN PCA normals of the points of a ragged batch (csrc/normals.hip, arithmetic csrc/normal_math.h): the unit
    eigenvector of the smallest eigenvalue of the covariance of every point's k neighbours.
    pts (total,3) fp32 and idx (total,k) int32 on the GPU, idx the LOCAL indices ``knn3_ragged`` returned; off (S+1):
    HOST integers (the caller built them) or a ``ragged.Clouds`` — they are checked here (ascending from 0 to total);
    host integers are uploaded with the tile table in one stream-ordered copy, a Clouds brings its device offsets and
    the tile table goes alone.  viewpoints (S,3) fp32 on the GPU or None.
    Returns normals (total,3) fp32 — canonical sign (largest component positive) without viewpoints, else flipped
    towards the segment's viewpoint — and, with ``want_scalars``, (normals, variation (total), gap (total)).
    A neighbourhood of coincident points and a segment of fewer than 3 points give zero normals and scalars."""
    require_cuda(pts, idx, viewpoints)
    off, clouds = _host_view("point_normals", off)
    pts = _f32c(pts, "pts")
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise ValueError("point_normals expects (total,3) points, got %s" % (tuple(pts.shape),))
    k = int(k)
    if not NORMALS_MIN_K <= k <= NORMALS_MAX_K:
        raise ValueError("point_normals: k must be %d .. %d, got %d" % (NORMALS_MIN_K, NORMALS_MAX_K, k))
    total = pts.shape[0]
    if idx.dtype != torch.int32:
        raise TypeError("idx must be int32, got %s" % idx.dtype)
    if tuple(idx.shape) != (total, k):
        raise ValueError("point_normals expects (%d,%d) neighbour indices, got %s" % (total, k, tuple(idx.shape)))
    off, S = _host_offsets("point_normals", off, total, k)
    dev = pts.device
    if viewpoints is not None:
        viewpoints = _f32c(viewpoints, "viewpoints")
        if tuple(viewpoints.shape) != (S, 3):
            raise ValueError("point_normals expects (%d,3) viewpoints, got %s" % (S, tuple(viewpoints.shape)))
    normals = torch.empty((total, 3), dtype=torch.float32, device=dev)
    variation = torch.empty(total, dtype=torch.float32, device=dev) if want_scalars else None
    gap = torch.empty(total, dtype=torch.float32, device=dev) if want_scalars else None
    if total > 0:
        lib = _lib.load()
        tile = lib.pn_point_normals_tile()
        tiles = (np.diff(off) + tile - 1) // tile
        ntile = int(tiles.sum())
        tile_seg = np.repeat(np.arange(S), tiles)
        tile_first = off[tile_seg] + (np.arange(ntile) - np.repeat(np.cumsum(tiles) - tiles, tiles)) * tile
        # host integers ride in front of the tile table, one copy; a Clouds has (or makes) its own
        ride = [] if clouds is not None else [off]
        table = _lib.h2d(np.concatenate(ride + [tile_seg, tile_first]).astype(np.int32), dev)
        off_d, tiles = (clouds.device_offsets(), table) if clouds is not None else (table, table[S + 1:])
        with _lib.on_device(dev):
            rc = lib.pn_point_normals_f32(ptr(pts), ptr(off_d), S, total, ptr(idx.contiguous()), k, ptr(viewpoints),
                                          ptr(tiles), ptr(tiles[ntile:]), ntile, ptr(normals), ptr(variation),
                                          ptr(gap), current_stream(dev))
        check(rc, "pn_point_normals_f32")
    return (normals, variation, gap) if want_scalars else normals


ORIENT_MIN_K, ORIENT_MAX_K = 1, 64


def _orient_args(who, pts, off, idx, k, normals):
    """The checks ``orient_normals`` and ``orient_normals_global`` share -> (pts, normals, host offsets int64, S, k,
    the Clouds given as off or None)."""
    require_cuda(pts, idx, normals)
    off, clouds = _host_view(who, off)
    pts = _f32c(pts, "pts")
    normals = _f32c(normals, "normals")
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise ValueError("%s expects (total,3) points, got %s" % (who, tuple(pts.shape),))
    total = pts.shape[0]
    if tuple(normals.shape) != (total, 3):
        raise ValueError("%s expects (%d,3) normals, got %s" % (who, total, tuple(normals.shape)))
    k = int(k)
    if not ORIENT_MIN_K <= k <= ORIENT_MAX_K:
        raise ValueError("%s: k must be %d .. %d, got %d" % (who, ORIENT_MIN_K, ORIENT_MAX_K, k))
    if idx.dtype != torch.int32:
        raise TypeError("idx must be int32, got %s" % idx.dtype)
    if tuple(idx.shape) != (total, k):
        raise ValueError("%s expects (%d,%d) neighbour indices, got %s" % (who, total, k, tuple(idx.shape)))
    off, S = _host_offsets(who, off, total, k)
    return pts, normals, off, S, k, clouds


def orient_normals(pts, off, idx, k, normals, want_flags=False):
    """Consistent orientation of the normals of a ragged batch without a viewpoint (csrc/orient.hip, definition
    csrc/orient_math.h): signs propagated along the minimum spanning forest of the k-NN graph under 1 - |n_i . n_j|,
    the topmost point of every connected component looking up.
    pts (total,3) fp32, idx (total,k) int32 — the LOCAL indices ``knn3_ragged`` returned — and normals (total,3) fp32
    on the GPU; off (S+1): HOST integers or a ``ragged.Clouds``, checked here (ascending from 0 to total, no segment
    above ``pn_orient_normals_max_points()``: ValueError); host integers are uploaded in one stream-ordered copy.
    Returns the oriented normals (total,3) — every row the input row, bit-identical or negated — and, with
    ``want_flags``, (normals, flip (total) int32 0/1, seed (total) int32: the local index of the component's seed).
    One launch, no host synchronisation; the same bits from run to run and for every batching.
    ``orient_normals_global`` computes the same on segments of any size."""
    pts, normals, off, S, k, clouds = _orient_args("orient_normals", pts, off, idx, k, normals)
    total = pts.shape[0]
    dev = pts.device
    out = torch.empty((total, 3), dtype=torch.float32, device=dev)
    flip = torch.empty(total, dtype=torch.int32, device=dev) if want_flags else None
    seed = torch.empty(total, dtype=torch.int32, device=dev) if want_flags else None
    if total > 0:
        lib = _lib.load()
        limit = lib.pn_orient_normals_max_points()
        if int(np.diff(off).max()) > limit:
            raise ValueError("orient_normals: a cloud of %d points; one workgroup orients at most %d points "
                             "(the global-memory engine, orient_normals_global or engine=\"global\" / \"auto\", has no "
                             "limit)" % (int(np.diff(off).max()), limit))
        off_d = _upload_offsets(off, clouds, dev)
        with _lib.on_device(dev):
            rc = lib.pn_orient_normals_f32(ptr(pts), ptr(off_d), S, total, ptr(idx.contiguous()), k, ptr(normals),
                                           ptr(out), ptr(flip), ptr(seed), current_stream(dev))
        check(rc, "pn_orient_normals_f32")
    return (out, flip, seed) if want_flags else out


def orient_normals_global(pts, off, idx, k, normals, want_flags=False):
    """``orient_normals`` on segments of any size: the same definition and the same bits from the global-memory engine
    (csrc/orient_global.hip, steps and schedule csrc/orient_global_math.h).  The same arguments, checks and results,
    without the limit on the points of a segment; total * k < 2^31.  The workspace (linear in total) is allocated
    here; ``pn_orient_normals_global_launches(largest segment)`` stream-ordered launches, no host synchronisation."""
    pts, normals, off, S, k, clouds = _orient_args("orient_normals_global", pts, off, idx, k, normals)
    total = pts.shape[0]
    dev = pts.device
    out = torch.empty((total, 3), dtype=torch.float32, device=dev)
    flip = torch.empty(total, dtype=torch.int32, device=dev) if want_flags else None
    seed = torch.empty(total, dtype=torch.int32, device=dev) if want_flags else None
    if total > 0:
        lib = _lib.load()
        wsz = lib.pn_orient_normals_global_workspace_bytes(total, S)
        ws = torch.empty(wsz, dtype=torch.uint8, device=dev)
        off_d = _upload_offsets(off, clouds, dev)
        with _lib.on_device(dev):
            rc = lib.pn_orient_normals_global_f32(ptr(pts), ptr(off_d), S, total, int(np.diff(off).max()),
                                                  ptr(idx.contiguous()), k, ptr(normals), ptr(out), ptr(flip),
                                                  ptr(seed), ptr(ws), wsz, current_stream(dev))
        check(rc, "pn_orient_normals_global_f32")
    return (out, flip, seed) if want_flags else out


def fps_ragged(pts, off, max_n, m, start=None, want_owner=False, want_radius=False):
    """Farthest-point sampling of every segment of a ragged batch (csrc/fps.hip, definition csrc/fps_math.h), exact and
    bit-reproducible.  pts (total,3) fp32, off (S+1) int32 device offsets, max_n >= the largest segment (a host
    integer) — or off a ``ragged.Clouds`` and max_n None —, m >= 1 samples per segment, start None (0) or (S,) int32
    LOCAL indices (clamped into the segment).
    Returns sample (S,m) int32 LOCAL indices in selection order, -1 past min(m, n) — and, with ``want_owner``, owner
    (total,) int32, the rank of every point's nearest sample, and dist (total,) fp32, the squared distance to it; with
    ``want_radius`` radius (S,m) fp32 last, the distance of every sample to the earlier ones when it was chosen (+inf
    first, NaN where sample is -1).  A segment that holds a non-finite coordinate: -1 and NaN throughout.
    ``pn_fps_launches(m)`` = m + 2 stream-ordered launches on a workspace allocated here, no host synchronisation."""
    require_cuda(start)
    pts, off, S, max_n = _device_offsets("fps_ragged", pts, off, max_n)
    m = int(m)
    if m < 1:
        raise ValueError("fps_ragged: m = %d (m >= 1)" % m)
    total = pts.shape[0]
    if total >= 2 ** 31:
        raise ValueError("fps_ragged: total = %d (below 2^31)" % total)
    if start is not None:
        if start.dtype != torch.int32:
            raise TypeError("start must be int32")
        if tuple(start.shape) != (S,):
            raise ValueError("fps_ragged: start must be (%d,), got %s" % (S, tuple(start.shape)))
        start = start.contiguous()
    dev = pts.device
    sample = torch.empty((max(S, 0), m), dtype=torch.int32, device=dev)
    radius = torch.empty((max(S, 0), m), dtype=torch.float32, device=dev) if want_radius else None
    owner = torch.empty(total, dtype=torch.int32, device=dev) if want_owner else None
    dist = torch.empty(total, dtype=torch.float32, device=dev) if want_owner else None
    if S > 0:
        lib = _lib.load()
        wsz = lib.pn_fps_workspace_bytes(total, S, m)
        ws = torch.empty(wsz, dtype=torch.uint8, device=dev)
        with _lib.on_device(dev):
            rc = lib.pn_fps_f32(ptr(pts), ptr(off()), S, total, max_n, m, ptr(start), ptr(sample), ptr(radius),
                                ptr(owner), ptr(dist), ptr(ws), wsz, current_stream(dev))
        check(rc, "pn_fps_f32")
    out = (sample,) + ((owner, dist) if want_owner else ()) + ((radius,) if want_radius else ())
    return out if len(out) > 1 else sample


VOXEL_OUTPUTS = ("centroid", "count", "first", "rep")


def voxel_ragged(pts, off, voxel, origin=None, want=VOXEL_OUTPUTS):
    """Voxel-grid downsampling of every segment of a ragged batch (csrc/voxel.hip, definition csrc/voxel_math.h), exact
    and bit-reproducible.  pts (total,3) fp32, off (S+1) int32 device offsets or a ``ragged.Clouds``, voxel (S,) fp32 on
    the device: the edge of the cubic cells of every segment, origin None (the per-axis minimum of the segment) or (S,3)
    fp32 on the device; ``want``: which of "centroid", "count", "first", "rep" to compute.
    Returns (owner (total,) int32: the number of every point's voxel — voxels are numbered by the ascending lowest
    point index they hold —, nvox (S,) int32: the voxels of every segment) and then, in the order of ``VOXEL_OUTPUTS``,
    the arrays named in ``want``: centroid (total,3) fp32, the exact mean of the voxel's points; count, first, rep
    (total,) int32: its points, its lowest point index, and the point nearest to the centroid (LOCAL indices).  The
    voxel arrays of a segment stand in the first nvox[s] entries of the segment's own rows, NaN / -1 behind them.
    nvox -1: the segment holds a non-finite coordinate; -2: the voxel is too small for the extent (a cell index outside
    -2^20 .. 2^20 - 1) or no positive finite number; both: owner -1, no voxel rows.
    ``pn_voxel_launches()`` = 7 stream-ordered launches on a workspace allocated here, no host synchronisation."""
    require_cuda(voxel, origin)
    pts, upload, S, _ = _device_offsets("voxel_ragged", pts, off, 0)
    unknown = [w for w in want if w not in VOXEL_OUTPUTS]
    if unknown:
        raise ValueError("voxel_ragged: want holds %s, got %r" % (", ".join(VOXEL_OUTPUTS), unknown))
    total, S, dev = pts.shape[0], max(S, 0), pts.device
    if total >= 2 ** 31:
        raise ValueError("voxel_ragged: total = %d (below 2^31)" % total)
    voxel = _f32c(voxel, "voxel")
    if tuple(voxel.shape) != (S,) or voxel.device != dev:
        raise ValueError("voxel_ragged: voxel must be (%d,) on %s, got %s on %s" % (S, dev, tuple(voxel.shape),
                                                                                      voxel.device))
    if origin is not None:
        origin = _f32c(origin, "origin")
        if tuple(origin.shape) != (S, 3) or origin.device != dev:
            raise ValueError("voxel_ragged: origin must be (%d,3) on %s, got %s on %s" % (S, dev, tuple(origin.shape),
                                                                                           origin.device))
    owner = torch.empty(total, dtype=torch.int32, device=dev)
    out = {"centroid": torch.empty((total, 3), dtype=torch.float32, device=dev) if "centroid" in want else None}
    for name in VOXEL_OUTPUTS[1:]:
        out[name] = torch.empty(total, dtype=torch.int32, device=dev) if name in want else None
    if total == 0:                                    # nothing to launch: every segment is empty
        nvox = torch.where((voxel > 0) & torch.isfinite(voxel), 0, -2).to(torch.int32)
    else:
        nvox = torch.empty(S, dtype=torch.int32, device=dev)
        lib = _lib.load()
        wsz = lib.pn_voxel_workspace_bytes(total, S)
        ws = torch.empty(wsz, dtype=torch.uint8, device=dev)
        with _lib.on_device(dev):
            rc = lib.pn_voxel_f32(ptr(pts), ptr(upload()), S, total, ptr(voxel), ptr(origin), ptr(owner), ptr(nvox),
                                  ptr(out["centroid"]), ptr(out["count"]), ptr(out["first"]), ptr(out["rep"]), ptr(ws),
                                  wsz, current_stream(dev))
        check(rc, "pn_voxel_f32")
    return (owner, nvox) + tuple(out[name] for name in VOXEL_OUTPUTS if name in want)


CLUSTER_OUTPUTS = ("count", "first", "ndrop")


def cluster_ragged(pts, off, radius, min_size=1, want=CLUSTER_OUTPUTS):
    """Euclidean cluster extraction of every segment of a ragged batch (csrc/cluster.hip, definition
    csrc/cluster_math.h), exact and bit-reproducible.  pts (total,3) fp32, off (S+1) int32 device offsets or a
    ``ragged.Clouds``, radius (S,) fp32 on the device: two points of a segment are joined when their fp32 squared
    distance is at most fl(r * r); min_size >= 1: a connected component of fewer points is dropped; ``want``: which of
    "count", "first", "ndrop" to compute.
    Returns (label (total,) int32: the number of every point's component — kept components are numbered by the ascending
    lowest point index they hold —, -1 for a point of a dropped component; ncomp (S,) int32: the kept components of
    every segment) and then, in the order of ``CLUSTER_OUTPUTS``, the arrays named in ``want``: count, first (total,)
    int32, the size and the lowest LOCAL index of the kept components in the first ncomp[s] entries of the segment's own
    rows, -1 behind them; ndrop (S,) int32, the points with label -1.  ncomp -1: the segment holds a non-finite
    coordinate; -2: the radius or its square is no positive finite number; both: label, count, first -1 throughout.
    The schedule is fixed by the largest segment of a Clouds, by total under plain offsets:
    ``pn_cluster_launches(max_n)`` stream-ordered launches on a workspace allocated here, no host synchronisation."""
    if not torch.is_tensor(radius):
        raise TypeError("cluster_ragged: radius must be a tensor, got %s" % type(radius).__name__)
    if isinstance(min_size, bool) or not isinstance(min_size, numbers.Integral) or not 1 <= min_size < 2 ** 31:
        raise ValueError("cluster_ragged: min_size must be an integer >= 1, got %r" % (min_size,))
    unknown = [w for w in want if w not in CLUSTER_OUTPUTS]
    if unknown:
        raise ValueError("cluster_ragged: want holds %s, got %r" % (", ".join(CLUSTER_OUTPUTS), unknown))
    require_cuda(radius)
    pts, upload, S, max_n = _device_offsets("cluster_ragged", pts, off, None if isinstance(off, Clouds) else 0)
    total, S, dev = pts.shape[0], max(S, 0), pts.device
    if total >= 2 ** 31:
        raise ValueError("cluster_ragged: total = %d (below 2^31)" % total)
    if not isinstance(off, Clouds):
        max_n = total
    radius = _f32c(radius, "radius")
    if tuple(radius.shape) != (S,) or radius.device != dev:
        raise ValueError("cluster_ragged: radius must be (%d,) on %s, got %s on %s" % (S, dev, tuple(radius.shape),
                                                                                        radius.device))
    label = torch.empty(total, dtype=torch.int32, device=dev)
    out = {name: torch.empty(total, dtype=torch.int32, device=dev) if name in want else None
           for name in CLUSTER_OUTPUTS[:2]}
    if total == 0:                                    # nothing to launch: every segment is empty
        r2 = radius * radius
        ncomp = torch.where((radius > 0) & torch.isfinite(radius) & (r2 > 0) & torch.isfinite(r2), 0, -2).to(torch.int32)
        out["ndrop"] = torch.zeros(S, dtype=torch.int32, device=dev) if "ndrop" in want else None
    else:
        ncomp = torch.empty(S, dtype=torch.int32, device=dev)
        out["ndrop"] = torch.empty(S, dtype=torch.int32, device=dev) if "ndrop" in want else None
        lib = _lib.load()
        wsz = lib.pn_cluster_workspace_bytes(total, S)
        ws = torch.empty(wsz, dtype=torch.uint8, device=dev)
        with _lib.on_device(dev):
            rc = lib.pn_cluster_f32(ptr(pts), ptr(upload()), S, total, int(max_n), ptr(radius), int(min_size),
                                    ptr(label), ptr(ncomp), ptr(out["count"]), ptr(out["first"]), ptr(out["ndrop"]),
                                    ptr(ws), wsz, current_stream(dev))
        check(rc, "pn_cluster_f32")
    return (label, ncomp) + tuple(out[name] for name in CLUSTER_OUTPUTS if name in want)


PLANE_OUTPUTS = ("dist",)
PLANE_MAX_H, PLANE_MAX_REFINE = 4096, 4


def _plane_axis(who, axis, max_angle):
    """axis and max_angle of ``plane_ragged`` -> (None, 0.0) or (the unit axis as three fp64 numbers, min_cos)."""
    if (axis is None) != (max_angle is None):
        raise ValueError("%s: axis and max_angle come together, got axis=%r, max_angle=%r" % (who, axis, max_angle))
    if axis is None:
        return None, 0.0
    try:
        a = [float(v) for v in axis]
    except (TypeError, ValueError):
        raise ValueError("%s: axis must be three numbers, got %r" % (who, axis))
    if len(a) != 3 or any(isinstance(v, bool) for v in axis):
        raise ValueError("%s: axis must be three numbers, got %r" % (who, axis))
    a = np.asarray(a, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        length = np.sqrt((a * a).sum())
    if not (np.isfinite(a).all() and np.isfinite(length) and length > 0.0):
        raise ValueError("%s: axis must be finite and not zero, got %r" % (who, axis))
    if isinstance(max_angle, bool) or not isinstance(max_angle, numbers.Real) or not 0.0 <= max_angle <= 90.0:
        raise ValueError("%s: max_angle must be a number of degrees 0 .. 90, got %r" % (who, max_angle))
    min_cos = min(1.0, max(0.0, math.cos(math.radians(float(max_angle)))))
    return np.ascontiguousarray(a / length), min_cos


def plane_ragged(pts, off, threshold, hypotheses=512, seed=0, refine=1, axis=None, max_angle=None, want=PLANE_OUTPUTS):
    """The dominant plane of every segment of a ragged batch (csrc/plane.hip, definition csrc/plane_math.h), exact and
    bit-reproducible.  pts (total,3) fp32, off (S+1) int32 device offsets or a ``ragged.Clouds``, threshold (S,) fp32
    on the device: a point is an inlier of a plane (n, d) iff |n . p + d| <= t in fp64; hypotheses 1 .. 4096 planes
    through three points drawn by a hash of (seed, h); refine 0 .. 4 rounds of a least-squares plane through the
    inliers, each taken only if it loses no inlier; axis (three host numbers, normalised here in fp64) with max_angle
    (degrees, 0 .. 90): only planes whose normal lies within max_angle of +-axis count; ``want``: () or ("dist",).
    Returns (plane (S,4) fp64: nx, ny, nz, d with |n| = 1 and the component of largest magnitude positive; count (S,)
    int32, the inliers; best (S,) int32, the winning hypothesis; inlier (total,) bool) and, with "dist" in ``want``, dist
    (total,) fp32, the signed distance of every point to the plane of its segment.  best -1: no valid hypothesis (fewer
    than three points, a collinear cloud, an axis that excludes every sample): count 0, plane zeros, no inlier, dist NaN.
    count -1: the segment holds a non-finite coordinate; -2: its threshold is no positive finite number; both as best -1.
    ``pn_plane_launches(refine)`` = 5 + 6 refine stream-ordered launches on a workspace allocated here, no host
    synchronisation."""
    who = "plane_ragged"
    if not torch.is_tensor(threshold):
        raise TypeError("%s: threshold must be a tensor, got %s" % (who, type(threshold).__name__))
    if isinstance(hypotheses, bool) or not isinstance(hypotheses, numbers.Integral) or not 1 <= hypotheses <= PLANE_MAX_H:
        raise ValueError("%s: hypotheses must be an integer 1 .. %d, got %r" % (who, PLANE_MAX_H, hypotheses))
    if isinstance(refine, bool) or not isinstance(refine, numbers.Integral) or not 0 <= refine <= PLANE_MAX_REFINE:
        raise ValueError("%s: refine must be an integer 0 .. %d, got %r" % (who, PLANE_MAX_REFINE, refine))
    if isinstance(seed, bool) or not isinstance(seed, numbers.Integral) or not -2 ** 63 <= seed < 2 ** 64:
        raise ValueError("%s: seed must be an integer of 64 bits, got %r" % (who, seed))
    axis, min_cos = _plane_axis(who, axis, max_angle)
    unknown = [w for w in want if w not in PLANE_OUTPUTS]
    if unknown:
        raise ValueError("%s: want holds %s, got %r" % (who, ", ".join(PLANE_OUTPUTS), unknown))
    for t in (pts, threshold) + (() if isinstance(off, Clouds) else (off,)):
        if torch.is_tensor(t) and not t.is_cuda:
            raise TypeError("%s: pts, off and threshold must be on the GPU, got a %s tensor" % (who, t.device))
    pts, upload, S, _ = _device_offsets(who, pts, off, 0)
    total, S, dev = pts.shape[0], max(S, 0), pts.device
    if total >= 2 ** 31:
        raise ValueError("%s: total = %d (below 2^31)" % (who, total))
    if S * int(hypotheses) >= 2 ** 31:
        raise ValueError("%s: segments * hypotheses = %d (below 2^31)" % (who, S * int(hypotheses)))
    threshold = _f32c(threshold, "threshold")
    if tuple(threshold.shape) != (S,) or threshold.device != dev:
        raise ValueError("%s: threshold must be (%d,) on %s, got %s on %s" % (who, S, dev, tuple(threshold.shape),
                                                                              threshold.device))
    inlier = torch.empty(total, dtype=torch.bool, device=dev)
    dist = torch.empty(total, dtype=torch.float32, device=dev) if "dist" in want else None
    if total == 0 or S == 0:                          # nothing to launch: every segment is empty
        plane = torch.zeros((S, 4), dtype=torch.float64, device=dev)
        count = torch.where((threshold > 0) & torch.isfinite(threshold), 0, -2).to(torch.int32)
        best = torch.full((S,), -1, dtype=torch.int32, device=dev)
    else:
        plane = torch.empty((S, 4), dtype=torch.float64, device=dev)
        count = torch.empty(S, dtype=torch.int32, device=dev)
        best = torch.empty(S, dtype=torch.int32, device=dev)
        lib = _lib.load()
        wsz = lib.pn_plane_workspace_bytes(total, S, int(hypotheses))
        ws = torch.empty(wsz, dtype=torch.uint8, device=dev)
        seed64 = int(seed) & (2 ** 64 - 1)
        with _lib.on_device(dev):
            rc = lib.pn_plane_f32(ptr(pts), ptr(upload()), S, total, ptr(threshold), int(hypotheses),
                                  seed64 - 2 ** 64 if seed64 >= 2 ** 63 else seed64, int(refine),
                                  None if axis is None else axis.ctypes.data, float(min_cos), ptr(plane), ptr(count),
                                  ptr(best), ptr(inlier), ptr(dist), ptr(ws), wsz, current_stream(dev))
        check(rc, "pn_plane_f32")
    return (plane, count, best, inlier) + ((dist,) if "dist" in want else ())


OUTLIER_MIN_K, OUTLIER_MAX_K = 1, 64


def outlier_stat(dist, off, k, std_ratio, want_index=True):
    """Statistical outlier removal over a ragged batch (csrc/outlier.hip, definition csrc/outlier_math.h), exact and
    bit-reproducible.  dist (total,k) fp32: the distances ``knn3_ragged`` (fp32) or ``knn3_grid`` returned with
    ``want_dist``; off (S+1) int32 device offsets or the ``ragged.Clouds`` the points were flattened by; 1 <= k <= 64;
    std_ratio finite and >= 0.
    Returns (avg (total) fp64: the mean distance of every point to its min(k, n) nearest, itself included; stats (S,3)
    fp64: mean, std and thr = mean + std_ratio * std of the valid (avg > 0) points of every segment; keep (total) bool:
    avg > 0 and avg < thr; kept (S) int32: the kept points per segment) and, with ``want_index``, index (total) int32
    last: the LOCAL indices of a segment's kept points, ascending, in the first kept[s] entries of its rows, -1 behind.
    A segment that holds a non-finite coordinate (NaN rows of dist): NaN, nothing kept.  An empty segment: mean and thr
    NaN, std 0.  ``pn_outlier_launches()`` = 6 stream-ordered launches on a workspace allocated here, no host
    synchronisation."""
    clouds = isinstance(off, Clouds)
    require_cuda(dist, None if clouds else off)
    dist = _f32c(dist, "dist")
    k = int(k)
    if not OUTLIER_MIN_K <= k <= OUTLIER_MAX_K:
        raise ValueError("outlier_stat: k must be %d .. %d, got %d" % (OUTLIER_MIN_K, OUTLIER_MAX_K, k))
    std_ratio = float(std_ratio)
    if not 0.0 <= std_ratio < float("inf"):
        raise ValueError("outlier_stat: std_ratio must be finite and not negative, got %r" % std_ratio)
    if dist.dim() != 2 or dist.shape[1] != k:
        raise ValueError("outlier_stat expects (total,%d) distances, got %s" % (k, tuple(dist.shape)))
    total = dist.shape[0]
    if total * k >= 2 ** 31:
        raise ValueError("outlier_stat: total * k = %d (below 2^31)" % (total * k))
    if clouds:
        if total != off.total or dist.device != off.flat.device:
            raise ValueError("outlier_stat: dist %s on %s does not belong to the Clouds given as off (%d points on %s)"
                             % (tuple(dist.shape), dist.device, off.total, off.flat.device))
        upload, S = off.device_offsets, off.S
    else:
        if off.dtype != torch.int32:
            raise TypeError("off must be int32")
        upload, S = off.contiguous, off.numel() - 1
    dev = dist.device
    S = max(S, 0)
    avg = torch.empty(total, dtype=torch.float64, device=dev)
    keep = torch.empty(total, dtype=torch.uint8, device=dev)
    index = torch.empty(total, dtype=torch.int32, device=dev) if want_index else None
    if total == 0:                                   # nothing to launch: every segment is empty
        stats = torch.full((S, 3), float("nan"), dtype=torch.float64, device=dev)
        stats[:, 1] = 0.0
        kept = torch.zeros(S, dtype=torch.int32, device=dev)
    else:
        stats = torch.empty((S, 3), dtype=torch.float64, device=dev)
        kept = torch.empty(S, dtype=torch.int32, device=dev)
    if total > 0 and S > 0:
        lib = _lib.load()
        wsz = lib.pn_outlier_workspace_bytes(total, S)
        ws = torch.empty(wsz, dtype=torch.uint8, device=dev)
        with _lib.on_device(dev):
            rc = lib.pn_outlier_stat_f32(ptr(dist), ptr(upload()), S, total, k, std_ratio, ptr(avg), ptr(stats),
                                         ptr(keep), ptr(kept), ptr(index), ptr(ws), wsz, current_stream(dev))
        check(rc, "pn_outlier_stat_f32")
    out = (avg, stats, keep.view(torch.bool), kept)
    return out + (index,) if want_index else out


def _i64c(t, name):
    if t.dtype != torch.int64:
        raise TypeError("%s must be int64, got %s" % (name, t.dtype))
    return t.contiguous()


def _graph_c(t, name):
    """A kNN graph: int64 (the API dtype) or int32 (the library's own, kernels.knn(..., int32=True))."""
    if t.dtype not in (torch.int64, torch.int32):
        raise TypeError("%s must be int64 or int32, got %s" % (name, t.dtype))
    return t.contiguous()


def transpose12(x):
    """(B,R,C) -> contiguous (B,C,R) through the LDS-tiled HIP transpose."""
    require_cuda(x)
    x = _f32c(x, "x")
    B, R, C = x.shape
    out = torch.empty((B, C, R), dtype=torch.float32, device=x.device)
    with _lib.on_device(x.device):
        rc = _lib.load().pn_transpose_f32(ptr(x), ptr(out), B, R, C, current_stream(x.device))
    check(rc, "pn_transpose_f32")
    return out


def edge_feature_fwd(xt, idx):
    """xt (B,N,C) point-major, idx (B,N,k) -> feat (B,N,k,2C) = cat(x_j - x_i, x_i)."""
    require_cuda(xt, idx)
    xt = _f32c(xt, "xt")
    idx = _i64c(idx, "idx")
    B, N, C = xt.shape
    k = idx.shape[2]
    feat = torch.empty((B, N, k, 2 * C), dtype=torch.float32, device=xt.device)
    with _lib.on_device(xt.device):
        rc = _lib.load().pn_edge_feature_fwd_f32(ptr(xt), ptr(idx), B, N, k, C, ptr(feat),
                                                 current_stream(xt.device))
    check(rc, "pn_edge_feature_fwd_f32")
    return feat


def edge_feature_bwd(gfeat, idx):
    """gfeat (B,N,k,2C) -> gradient w.r.t. xt (B,N,C)."""
    require_cuda(gfeat, idx)
    gfeat = _f32c(gfeat, "gfeat")
    idx = _i64c(idx, "idx")
    B, N, k, C2 = gfeat.shape
    C = C2 // 2
    gxt = torch.empty((B, N, C), dtype=torch.float32, device=gfeat.device)
    lib = _lib.load()
    wsz = lib.pn_edgeconv_bwd_workspace(B, N, k)
    ws = torch.empty(wsz, dtype=torch.uint8, device=gfeat.device)
    with _lib.on_device(gfeat.device):
        rc = lib.pn_edge_feature_bwd_f32(ptr(gfeat), ptr(idx), B, N, k, C, ptr(gxt), ptr(ws), wsz,
                                         current_stream(gfeat.device))
    check(rc, "pn_edge_feature_bwd_f32")
    return gxt


def edgeconv_reduce_fwd(PQ, idx, gamma, groups, per_sample):
    """PQ (B,N,2*Cout) = [P | Q], idx (B,N,k).  Returns yext, argk (uint8), s1 (all (B,N,Cout))
    and the fp64 group moments stats ((B or 1), groups, 2) of y = P[j] + Q[i] over all edges."""
    require_cuda(PQ, idx, gamma)
    PQ = _f32c(PQ, "PQ")
    idx = _graph_c(idx, "idx")
    gamma = _f32c(gamma, "gamma")
    B, N, C2 = PQ.shape
    Cout = C2 // 2
    k = idx.shape[2]
    dev = PQ.device
    yext = torch.empty((B, N, Cout), dtype=torch.float32, device=dev)
    s1 = torch.empty((B, N, Cout), dtype=torch.float32, device=dev)
    argk = torch.empty((B, N, Cout), dtype=torch.uint8, device=dev)
    stats = torch.empty((B if per_sample else 1, groups, 2), dtype=torch.float64, device=dev)
    lib = _lib.load()
    wsz = lib.pn_edgeconv_reduce_workspace(B, N, Cout, groups)
    ws = torch.empty(wsz, dtype=torch.uint8, device=dev)
    fn = lib.pn_edgeconv_reduce_fwd_i32 if idx.dtype == torch.int32 else lib.pn_edgeconv_reduce_fwd_f32
    with _lib.on_device(dev):
        rc = fn(ptr(PQ), ptr(idx), ptr(gamma), B, N, k, Cout, groups, int(per_sample), ptr(yext), ptr(argk),
                ptr(s1), ptr(stats), ptr(ws), wsz, current_stream(dev))
    check(rc, "pn_edgeconv_reduce_fwd")
    return yext, argk, s1, stats


def moments(stats, count, eps):
    """fp64 (sum, sum of squares) -> fp32 (mean, rstd) per group."""
    require_cuda(stats)
    n = stats.numel() // 2
    mean = torch.empty(stats.shape[:-1], dtype=torch.float32, device=stats.device)
    rstd = torch.empty_like(mean)
    with _lib.on_device(stats.device):
        rc = _lib.load().pn_moments_f32(ptr(stats), n, float(count), float(eps), ptr(mean), ptr(rstd),
                                        current_stream(stats.device))
    check(rc, "pn_moments_f32")
    return mean, rstd


def edgeconv_finalize_fwd(yext, mean, rstd, gamma, beta, groups, per_sample, slope):
    """out (B,Cout,N) = LeakyReLU(gamma * (yext - mean) * rstd + beta), channel-first."""
    require_cuda(yext)
    B, N, Cout = yext.shape
    out = torch.empty((B, Cout, N), dtype=torch.float32, device=yext.device)
    with _lib.on_device(yext.device):
        rc = _lib.load().pn_edgeconv_finalize_fwd_f32(ptr(yext), ptr(_f32c(mean, "mean")),
                                                      ptr(_f32c(rstd, "rstd")), ptr(_f32c(gamma, "gamma")),
                                                      ptr(_f32c(beta, "beta")), B, N, Cout, groups,
                                                      int(per_sample), float(slope), ptr(out),
                                                      current_stream(yext.device))
    check(rc, "pn_edgeconv_finalize_fwd_f32")
    return out


def edgeconv_bwd_prep(gout, yext, mean, rstd, gamma, beta, groups, per_sample, slope):
    """gout (B,Cout,N) -> gz, yhat as (B,N,Cout)."""
    require_cuda(gout, yext)
    gout = _f32c(gout, "gout")
    B, N, Cout = yext.shape
    gz = torch.empty_like(yext)
    yhat = torch.empty_like(yext)
    with _lib.on_device(yext.device):
        rc = _lib.load().pn_edgeconv_bwd_prep_f32(ptr(gout), ptr(yext), ptr(mean), ptr(rstd),
                                                  ptr(_f32c(gamma, "gamma")), ptr(_f32c(beta, "beta")), B, N,
                                                  Cout, groups, int(per_sample), float(slope), ptr(gz),
                                                  ptr(yhat), current_stream(yext.device))
    check(rc, "pn_edgeconv_bwd_prep_f32")
    return gz, yhat


def edgeconv_csr_build(idx):
    """The transposed kNN graph of idx (B,N,k) for edgeconv_bwd(..., csr=...): a workspace tensor.  Depends on idx
    alone — graph.py builds it during the forward pass on a side stream."""
    require_cuda(idx)
    idx = _graph_c(idx, "idx")
    B, N, k = idx.shape
    lib = _lib.load()
    wsz = lib.pn_edgeconv_bwd_workspace(B, N, k)
    ws = torch.empty(wsz, dtype=torch.uint8, device=idx.device)
    with _lib.on_device(idx.device):
        rc = lib.pn_edgeconv_csr_build(ptr(idx), int(idx.dtype == torch.int32), B, N, k, ptr(ws), wsz,
                                       current_stream(idx.device))
    check(rc, "pn_edgeconv_csr_build")
    return ws


def edgeconv_bwd(PQ, idx, t, s1, argk, mean, rstd, c1c2, groups, per_sample, dense, csr=None):
    """Edge-level normalisation gradient -> dPQ (B,N,2*Cout); see csrc/edge.hip.  ``csr``: the workspace of
    edgeconv_csr_build(idx) (the transposed graph, already built), else it is built here."""
    require_cuda(PQ, idx, t)
    B, N, C2 = PQ.shape
    Cout = C2 // 2
    k = idx.shape[2]
    dPQ = torch.empty_like(PQ)
    lib = _lib.load()
    wsz = lib.pn_edgeconv_bwd_workspace(B, N, k)
    idx = _graph_c(idx, "idx")
    if csr is not None:
        if csr.numel() < wsz:
            raise ValueError("edgeconv_bwd: the prebuilt graph does not belong to this idx")
        with _lib.on_device(PQ.device):
            rc = lib.pn_edgeconv_bwd_prebuilt(ptr(PQ), ptr(idx), int(idx.dtype == torch.int32), ptr(_f32c(t, "t")), ptr(s1),
                                              ptr(argk), ptr(mean), ptr(rstd), ptr(_f32c(c1c2, "c1c2")), B, N, k, Cout,
                                              groups, int(per_sample), int(dense), ptr(dPQ), ptr(csr), csr.numel(),
                                              current_stream(PQ.device))
        check(rc, "pn_edgeconv_bwd_prebuilt")
        return dPQ
    ws = torch.empty(wsz, dtype=torch.uint8, device=PQ.device)
    fn = lib.pn_edgeconv_bwd_i32 if idx.dtype == torch.int32 else lib.pn_edgeconv_bwd_f32
    with _lib.on_device(PQ.device):
        rc = fn(ptr(PQ), ptr(idx), ptr(_f32c(t, "t")), ptr(s1), ptr(argk), ptr(mean), ptr(rstd),
                ptr(_f32c(c1c2, "c1c2")), B, N, k, Cout, groups, int(per_sample), int(dense), ptr(dPQ), ptr(ws), wsz,
                current_stream(PQ.device))
    check(rc, "pn_edgeconv_bwd")
    return dPQ


def dot_select(q, c, k, want_value):
    """q (B,Nq,C), c (B,Nc,C) point-major.  Returns (result, flags) where result is either the
    (B,Nq,k) int64 indices of the k largest dot products (best first) or the (B,Nq) k-th largest
    dot product, and flags (B,Nq) int32 marks rows the caller must recompute.  Returns None when
    the shape is outside the kernel's fast path."""
    require_cuda(q, c)
    q = _f32c(q, "q")
    c = _f32c(c, "c")
    B, Nq, C = q.shape
    Nc = c.shape[1]
    lib = _lib.load()
    wsz = lib.pn_dot_select_workspace(B, C, Nq, Nc, int(k), int(bool(want_value)))
    if wsz == 0:
        return None
    dev = q.device
    ws = torch.empty(wsz, dtype=torch.uint8, device=dev)
    flags = torch.empty((B, Nq), dtype=torch.int32, device=dev)
    if want_value:
        out = torch.empty((B, Nq), dtype=torch.float32, device=dev)
        args = (None, ptr(out))
    else:
        out = torch.empty((B, Nq, k), dtype=torch.int64, device=dev)
        args = (ptr(out), None)
    with _lib.on_device(dev):
        rc = lib.pn_dot_select_f32(ptr(q), Nq, ptr(c), Nc, B, C, int(k), args[0], args[1], ptr(flags),
                                   ptr(ws), wsz, current_stream(dev))
    check(rc, "pn_dot_select_f32")
    return out, flags


def dot_kth_x3(q, c, k):
    """K-th largest dot product between the rows of q (B,Nq,C) and c (B,Nc,C) with both distance
    passes in bf16 x 3 arithmetic (fp32-grade, |error| ~1e-7 on unit rows): (values (B,Nq), flags),
    or None outside that path (C <= 128, Nc >= 2048, the fast-path shape rules)."""
    require_cuda(q, c)
    q, c = _f32c(q, "q"), _f32c(c, "c")
    B, Nq, C = q.shape
    Nc = c.shape[1]
    lib = _lib.load()
    wsz = lib.pn_dot_select_workspace(B, C, Nq, Nc, int(k), 1)
    if wsz == 0:
        return None
    dev = q.device
    ws = torch.empty(wsz, dtype=torch.uint8, device=dev)
    flags = torch.empty((B, Nq), dtype=torch.int32, device=dev)
    out = torch.empty((B, Nq), dtype=torch.float32, device=dev)
    with _lib.on_device(dev):
        rc = lib.pn_dot_kth_x3_f32(ptr(q), Nq, ptr(c), Nc, B, C, int(k), ptr(out), ptr(flags), ptr(ws), wsz,
                                   current_stream(dev))
    if rc == _lib.CONSTANTS["PN_ERR_UNSUPPORTED"]:      # shape outside the split passes
        return None
    check(rc, "pn_dot_kth_x3_f32")
    return out, flags


def dot_kth_unit(q, c_image, Nc, k):
    """K-th largest dot product between the unit rows of q (B,Nq,128) and the candidates whose
    fp16 x 2 tile images are ``c_image`` (meanshift_h2_split): (values (B,Nq), flags) with the
    distance passes on the fp16 matrix cores (|error| ~1e-7), or None outside the fast path."""
    require_cuda(q)
    q = _f32c(q, "q")
    B, Nq, C = q.shape
    lib = _lib.load()
    wsz = lib.pn_dot_select_workspace(B, C, Nq, int(Nc), int(k), 1)
    if wsz == 0 or C != 128:
        return None
    dev = q.device
    ws = torch.empty(wsz, dtype=torch.uint8, device=dev)
    flags = torch.empty((B, Nq), dtype=torch.int32, device=dev)
    out = torch.empty((B, Nq), dtype=torch.float32, device=dev)
    with _lib.on_device(dev):
        rc = lib.pn_dot_kth_unit_h2_f32(ptr(q), Nq, ptr(c_image), int(Nc), B, C, int(k), ptr(out), ptr(flags),
                                        ptr(ws), wsz, current_stream(dev))
    check(rc, "pn_dot_kth_unit_h2_f32")
    return out, flags


class MeanShiftWorkspace:
    """Scratch buffers of the mean-shift kernels for one (B,N,D) problem, allocated once per
    mean_shift call and reused by every iteration."""

    def __init__(self, B, N, D, device, backward=False, exact_f32=True):
        lib = _lib.load()
        self.B, self.N, self.D = B, N, D
        self.Np = (N + 63) // 64 * 64
        self.S = lib.pn_meanshift_slices(B, N)
        f = dict(dtype=torch.float32, device=device)
        self.opart = torch.empty((B, self.S, N, D), **f)
        self.rpart = torch.empty((B, self.S, N), **f)
        self.x3_imgs = self.h2_imgs = None      # tile images of the split backwards, made by their first step
        if backward:
            self.gu = torch.empty((B, N, D), **f)
            # row scalars (+ the per-tile maxima of the fp16 path)
            self.cs = torch.empty(3 * B * N + B * (self.Np // 32), **f)
            self.opart_x = torch.empty((B, self.S, N, D), **f)
            if exact_f32:   # the bf16 x 3 path needs neither go nor the channel-first copies
                self.go = torch.empty((B, N, D), **f)
                self.qt = torch.empty((B, D, self.Np), **f)
                self.gut = torch.empty((B, D, self.Np), **f)


def meanshift_pack(x):
    require_cuda(x)
    x = _f32c(x, "x")
    B, N, D = x.shape
    Np = (N + 63) // 64 * 64
    xt = torch.empty((B, D, Np), dtype=torch.float32, device=x.device)
    with _lib.on_device(x.device):
        rc = _lib.load().pn_meanshift_pack_f32(ptr(x), B, N, D, ptr(xt), current_stream(x.device))
    check(rc, "pn_meanshift_pack_f32")
    return xt


def meanshift_x3_split(x):
    """x (B,N,128) -> pre-split bf16 x 3 tile images for the matrix-core path."""
    require_cuda(x)
    x = _f32c(x, "x")
    B, N, D = x.shape
    lib = _lib.load()
    img = torch.empty(lib.pn_meanshift_x3_image_bytes(B, N), dtype=torch.uint8, device=x.device)
    with _lib.on_device(x.device):
        rc = lib.pn_meanshift_x3_split_f32(ptr(x), B, N, D, ptr(img), current_stream(x.device))
    check(rc, "pn_meanshift_x3_split_f32")
    return img


def meanshift_x3_tileinfo(z):
    """z (B,N,128) unit rows -> (centres (B,T,2,128), angular radii (B,T,2), row counts (B,T,2)) of
    the two bounding caps of every 32-row tile, T = align_up(N, 64) / 32 (radius < 0: empty cap): the
    geometry the block-sparse plan is derived from."""
    require_cuda(z)
    z = _f32c(z, "z")
    B, N, D = z.shape
    T = (N + 63) // 64 * 2
    cen = torch.empty((B, T, 2, D), dtype=torch.float32, device=z.device)
    rho = torch.empty((B, T, 2), dtype=torch.float32, device=z.device)
    cnt = torch.empty((B, T, 2), dtype=torch.float32, device=z.device)
    with _lib.on_device(z.device):
        rc = _lib.load().pn_meanshift_x3_tileinfo_f32(ptr(z), B, N, D, ptr(cen), ptr(rho), ptr(cnt),
                                                      current_stream(z.device))
    check(rc, "pn_meanshift_x3_tileinfo_f32")
    return cen, rho, cnt


def kmeans_assign(x, cen):
    """x (B,N,128), cen (B,K,128) -> (B,N) int32: the centre with the largest dot product (ties -> smaller index)."""
    require_cuda(x, cen)
    x, cen = _f32c(x, "x"), _f32c(cen, "cen")
    B, N, D = x.shape
    lab = torch.empty((B, N), dtype=torch.int32, device=x.device)
    with _lib.on_device(x.device):
        rc = _lib.load().pn_kmeans_assign_f32(ptr(x), ptr(cen), B, N, D, cen.shape[1], ptr(lab), current_stream(x.device))
    check(rc, "pn_kmeans_assign_f32")
    return lab


def kmeans_centres(x, lab, old):
    """Normalised sums of the points of every cell (lab (B,N) int32 from kmeans_assign); an empty cell keeps
    ``old`` (B,K,128)."""
    require_cuda(x, lab, old)
    x, old = _f32c(x, "x"), _f32c(old, "old")
    if lab.dtype != torch.int32 or not lab.is_contiguous():
        raise ValueError("kmeans_centres: lab must be a contiguous int32 tensor")
    B, N, D = x.shape
    cen = torch.empty_like(old)
    with _lib.on_device(x.device):
        rc = _lib.load().pn_kmeans_centres_f32(ptr(x), ptr(lab), ptr(old), B, N, D, old.shape[1], ptr(cen),
                                               current_stream(x.device))
    check(rc, "pn_kmeans_centres_f32")
    return cen


CELL_ORDER_MAX_CELLS = 768


def cell_order(rank, home, fine):
    """Stable argsort of rank[home[fine]] * F + fine as ONE counting-sort launch: rank (B,P), home (B,F), fine (B,N),
    all int32 -> (B,N) int64.  F <= CELL_ORDER_MAX_CELLS."""
    require_cuda(rank, home, fine)
    for t, nm in ((rank, "rank"), (home, "home"), (fine, "fine")):
        if t.dtype != torch.int32 or not t.is_contiguous():
            raise ValueError("cell_order: %s must be a contiguous int32 tensor" % nm)
    B, N = fine.shape
    perm = torch.empty((B, N), dtype=torch.int64, device=fine.device)
    with _lib.on_device(fine.device):
        rc = _lib.load().pn_cell_order_i32(ptr(rank), ptr(home), ptr(fine), B, N, rank.shape[1], home.shape[1],
                                           ptr(perm), current_stream(fine.device))
    check(rc, "pn_cell_order_i32")
    return perm


def meanshift_chain_order(sim, as_long=True):
    """sim (B,128,128) similarities of cell centres -> (B,128) int64 (int32 with ``as_long=False``) position of
    every cell in the greedy nearest-neighbour chain that starts at cell 0."""
    require_cuda(sim)
    sim = _f32c(sim, "sim")
    B, P, _ = sim.shape
    rank = torch.empty((B, P), dtype=torch.int32, device=sim.device)
    with _lib.on_device(sim.device):
        rc = _lib.load().pn_meanshift_chain_order_f32(ptr(sim), B, P, ptr(rank), current_stream(sim.device))
    check(rc, "pn_meanshift_chain_order_f32")
    return rank.long() if as_long else rank


def meanshift_x3_plan_bytes(B, N):
    return int(_lib.load().pn_meanshift_x3_plan_bytes(B, N))


def meanshift_x3_plan_buffer(B, N, iterations, device):
    """One buffer for the plans of ``iterations`` launches: plan t lives at t * core bytes, the scratch of the plan
    call (dead once it returns) of plan t overlaps the plans still to be written, ONE scratch region at the end.
    Returns (buffer, [views of plan_bytes each], core bytes)."""
    lib = _lib.load()
    full, core = int(lib.pn_meanshift_x3_plan_bytes(B, N)), int(lib.pn_meanshift_x3_plan_core_bytes(B, N))
    buf = torch.empty(iterations * core + (full - core), dtype=torch.uint8, device=device)
    return buf, [buf[t * core:t * core + full] for t in range(iterations)], core


def meanshift_x3_plan(q_info, x_info, bsq, N, rel_eps=1e-9, out=None):
    """Block-sparse plan of one iteration (which tile pairs can contribute more than ``rel_eps`` of
    the smallest row sum): an opaque byte tensor for meanshift_x3_iter_fwd / _bwd.  The product passes
    mean_shift.PLAN_REL_EPS (1e-6) for the forward-only training path and PLAN_REL_EPS_DENSE_BWD (1e-9)
    where a dense backward reuses the plan; the default here is the tighter one.  ``out``: a contiguous uint8
    tensor of meanshift_x3_plan_bytes(B, N) to write into (a row of the buffer that holds all plans of a call)."""
    cq, rq = q_info[0], q_info[1]
    cx, rx = x_info[0], x_info[1]
    nx = x_info[2] if len(x_info) > 2 else None      # rows of the data caps (None: conservative bounds)
    B = cq.shape[0]
    lib = _lib.load()
    plan = out if out is not None else torch.empty(lib.pn_meanshift_x3_plan_bytes(B, N), dtype=torch.uint8,
                                                   device=cq.device)
    with _lib.on_device(cq.device):
        rc = lib.pn_meanshift_x3_plan_f32(ptr(cq), ptr(rq), ptr(cx), ptr(rx), ptr(nx), ptr(bsq), B, N, float(rel_eps),
                                          ptr(plan), current_stream(cq.device))
    check(rc, "pn_meanshift_x3_plan_f32")
    return plan


def meanshift_x3_nearest(xq, xc, q_info, c_info, perm=None):
    """arg-max_j xq_i . xc_j for unit rows xq, xc (B,N,128) given in one common locality order, with
    their tile caps (meanshift_x3_tileinfo); perm (B,N) int64 position -> original index.  Returns
    (B,N) int64 indexed by / naming ORIGINAL indices: exactly dot_select(xq, xc, 1) of the unpermuted
    tensors (fp32 fma chains, ties to the smaller index), evaluated on the tile pairs that can hold
    a maximum only."""
    require_cuda(xq, xc)
    xq, xc = _f32c(xq, "xq"), _f32c(xc, "xc")
    B, N, D = xq.shape
    lib = _lib.load()
    out = torch.empty((B, N), dtype=torch.int64, device=xq.device)
    wsz = lib.pn_meanshift_x3_plan_bytes(B, N)
    ws = torch.empty(wsz, dtype=torch.uint8, device=xq.device)
    if perm is not None:
        perm = _i64c(perm, "perm")
    with _lib.on_device(xq.device):
        rc = lib.pn_meanshift_x3_nearest_f32(ptr(xq), ptr(xc), ptr(q_info[0]), ptr(q_info[1]), ptr(c_info[0]),
                                             ptr(c_info[1]), ptr(perm), B, N, D, ptr(out), ptr(ws), wsz,
                                             current_stream(xq.device))
    check(rc, "pn_meanshift_x3_nearest_f32")
    return out


def meanshift_x3_plan_stats(plan, B, N):
    """(active fraction of tile pairs, of pass-0 / pass-1 / pass-2 block x tile pairs) — diagnostics."""
    T = (N + 63) // 64 * 2
    nb0, nb1, nb2 = -(-N // 256), -(-N // 128), -(-N // 256)
    oc = (B * T * T + 255) // 256 * 256
    pairs = plan[:B * T * T].float().mean().item()
    counts = plan[oc:oc + B * (nb0 + nb1 + nb2) * 4].view(torch.int32).reshape(B, -1).float()
    return (pairs, counts[:, :nb0].mean().item() / T, counts[:, nb0:nb0 + nb1].mean().item() / T,
            counts[:, nb0 + nb1:].mean().item() / T)


def meanshift_x3_plan_visited(plans, B, N):
    """Device scalar: the share of the N^2 tile pairs the plans keep, averaged over the plans — what
    the planned launches execute relative to dense ones (their duration follows it: measured 0.73 of
    the dense launch at 0.71 of the pairs, 0.83 at 0.85).  No synchronisation (the caller downloads
    it with something it waits for anyway)."""
    T = (N + 63) // 64 * 2
    n = B * T * T
    if isinstance(plans, tuple):
        # all plans of the call in one buffer (meanshift_x3_plan_buffer), ``core`` bytes apart: ONE reduction (the
        # flags are 0 / 1 bytes, the fp32 sum of <= 2^24 of them is exact in any order)
        buf, count, core = plans
        return buf.as_strided((count, n), (core, 1)).sum(dtype=torch.float32) / float(n * count)
    return torch.stack([p[:n].sum(dtype=torch.float32) for p in plans]).mean() / float(n)


KERNEL_GAUSSIAN = _lib.CONSTANTS["PN_MS_KERNEL_GAUSSIAN"]
KERNEL_EPANECHNIKOV = _lib.CONSTANTS["PN_MS_KERNEL_EPANECHNIKOV"]


def _ms_out(who, q, out):
    """The (y (B,N,D), rsum (B,N), unorm (B,N)) triple a forward step on q (B,N,D) writes: ``out`` checked, or
    allocated when it is None."""
    B, N, D = q.shape
    if out is None:
        return (torch.empty_like(q), torch.empty((B, N), dtype=torch.float32, device=q.device),
                torch.empty((B, N), dtype=torch.float32, device=q.device))
    for t, shp in zip(out, ((B, N, D), (B, N), (B, N))):
        if tuple(t.shape) != shp or t.dtype != torch.float32 or not t.is_contiguous() or t.device != q.device:
            raise ValueError("%s: out tensors must be contiguous fp32 of shapes (B,N,D), (B,N), (B,N)" % who)
    y, rsum, unorm = out
    return y, rsum, unorm


def meanshift_x3_iter_fwd(q, x_image, bsq, ws, plan=None, out=None, want_info=False, kind=KERNEL_GAUSSIAN):
    """``out`` = (y (B,N,D), rsum (B,N), unorm (B,N)) contiguous fp32 tensors to write into (slices of
    the buffers that keep all iterates of a call together), or None: allocated here.  ``want_info``: also
    return meanshift_x3_tileinfo(y) — the caps come out of the launch that combines the partial results.
    ``kind``: the kernel profile; the Epanechnikov kernel launches dense (the library refuses it a plan) and
    returns no caps."""
    B, N, D = q.shape
    if kind != KERNEL_GAUSSIAN and want_info:
        raise ValueError("meanshift_x3_iter_fwd: the caps of the iterate feed the plans, which are Gaussian-only")
    y, rsum, unorm = _ms_out("meanshift_x3_iter_fwd", q, out)
    if not want_info:
        with _lib.on_device(q.device):
            rc = _lib.load().pn_meanshift_x3_iter_fwd_kind_f32(ptr(q), ptr(x_image), ptr(bsq), B, N, D, ptr(ws.opart),
                                                               ptr(ws.rpart), ptr(y), ptr(rsum), ptr(unorm),
                                                               ptr(plan), int(kind), current_stream(q.device))
        check(rc, "pn_meanshift_x3_iter_fwd_kind_f32")
        return y, rsum, unorm
    T = (N + 63) // 64 * 2
    info = (torch.empty((B, T, 2, D), dtype=torch.float32, device=q.device),
            torch.empty((B, T, 2), dtype=torch.float32, device=q.device),
            torch.empty((B, T, 2), dtype=torch.float32, device=q.device))
    with _lib.on_device(q.device):
        rc = _lib.load().pn_meanshift_x3_iter_fwd_info_f32(ptr(q), ptr(x_image), ptr(bsq), B, N, D, ptr(ws.opart),
                                                           ptr(ws.rpart), ptr(y), ptr(rsum), ptr(unorm),
                                                           ptr(plan), ptr(info[0]), ptr(info[1]), ptr(info[2]),
                                                           current_stream(q.device))
    check(rc, "pn_meanshift_x3_iter_fwd_info_f32")
    return y, rsum, unorm, info


def meanshift_x3_iter_bwd(gy, y, q, x, x_image, rsum, unorm, bsq, ws, gx, plan=None, kind=KERNEL_GAUSSIAN):
    """bf16 x 3 counterpart of meanshift_iter_bwd: returns dL/dq, adds into ``gx``.  ``kind``: the kernel
    profile of the forward call."""
    B, N, D = x.shape
    gy = _f32c(gy, "gy")
    gq = torch.empty_like(x)
    lib = _lib.load()
    if ws.x3_imgs is None:
        nbytes = lib.pn_meanshift_x3_image_bytes(B, N)
        ws.x3_imgs = [torch.empty(nbytes, dtype=torch.uint8, device=x.device) for _ in range(2)]
    im = ws.x3_imgs
    with _lib.on_device(x.device):
        rc = lib.pn_meanshift_x3_iter_bwd_kind_f32(ptr(gy), ptr(y), ptr(q), ptr(x), ptr(x_image), ptr(rsum),
                                                   ptr(unorm), ptr(bsq), B, N, D, ptr(ws.gu), ptr(ws.cs),
                                                   ptr(im[0]), ptr(im[1]), ptr(ws.opart), ptr(ws.opart_x), ptr(gq),
                                                   ptr(gx), ptr(plan), int(kind), current_stream(x.device))
    check(rc, "pn_meanshift_x3_iter_bwd_kind_f32")
    return gq


class MeanShiftWWorkspace:
    """The one scratch buffer of the width-32 / width-64 mean-shift kernels (csrc/meanshift_w.hip) for a
    (B,N,D) problem, shared by the iterations of a call.  The buffer also holds the tile images of the data
    ``x``; ``image_of`` remembers WHICH tensor they were built from (the tensor object itself, kept alive here so
    that its address cannot be handed to another tensor, and its version counter), so that a later call with
    the same, unmodified ``x`` skips that launch and a call with any other ``x`` — or the same one written to
    in place since — rebuilds them.  ``reset()`` forgets them."""

    def __init__(self, B, N, D, device, backward=False):
        nbytes = int(_lib.load().pn_meanshift_w_workspace(B, N, D, int(bool(backward))))
        if nbytes == 0:
            raise ValueError("meanshift_w: no kernel for shape (%d,%d,%d) (width 32 or 64)" % (B, N, D))
        self.B, self.N, self.D, self.backward = B, N, D, bool(backward)
        self.buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
        self.image_of = None

    def reset(self):
        self.image_of = None

    def holds_image_of(self, x):
        return self.image_of is not None and self.image_of[0] is x and self.image_of[1] == x._version

    def took_image_of(self, x):
        self.image_of = (x, x._version)


def _msw_rows(t, name, B, N, device):
    """A per-row operand of the width kernels: contiguous fp32 (B,N) on the launch device."""
    if t.dtype != torch.float32 or tuple(t.shape) != (B, N) or not t.is_contiguous() or t.device != device:
        raise ValueError("%s must be a contiguous float32 (%d,%d) tensor on %s" % (name, B, N, device))
    return t


def _msw_bsq(bsq, B, device):
    if bsq.dtype != torch.float32 or bsq.numel() != B or bsq.dim() != 1 or bsq.device != device:
        raise ValueError("bsq must be a float32 (%d,) tensor on %s" % (B, device))
    return bsq.contiguous()


def meanshift_w_iter_fwd(q, x, bsq, ws, out=None, kind=KERNEL_GAUSSIAN):
    """One mean-shift iteration at width 32 or 64: q (B,N,D) the current iterate, x (B,N,D) the data, bsq
    (B) squared bandwidths -> (y (B,N,D), rsum (B,N), unorm (B,N)), the triple meanshift_x3_iter_fwd
    returns.  ``out``: contiguous fp32 tensors of those shapes to write into.  The tile images of ``x`` in the
    workspace are reused when they were built from this very ``x`` (see MeanShiftWWorkspace), rebuilt otherwise.
    ``kind``: the kernel profile (KERNEL_GAUSSIAN / KERNEL_EPANECHNIKOV)."""
    require_cuda(q, x, bsq)
    q, x = _f32c(q, "q"), _f32c(x, "x")
    B, N, D = x.shape
    bsq = _msw_bsq(bsq, B, x.device)
    if tuple(q.shape) != (B, N, D) or (ws.B, ws.N, ws.D, ws.backward) != (B, N, D, False):
        raise ValueError("meanshift_w_iter_fwd: q, x (B,N,D) and a forward workspace of that shape")
    y, rsum, unorm = _ms_out("meanshift_w_iter_fwd", q, out)
    with _lib.on_device(q.device):
        rc = _lib.load().pn_meanshift_w_iter_fwd_kind_f32(ptr(q), ptr(x), ptr(bsq), B, N, D, ptr(y), ptr(rsum),
                                                          ptr(unorm), ptr(ws.buf), ws.buf.numel(),
                                                          int(ws.holds_image_of(x)), int(kind),
                                                          current_stream(q.device))
    check(rc, "pn_meanshift_w_iter_fwd_kind_f32")
    ws.took_image_of(x)
    return y, rsum, unorm


def meanshift_w_iter_bwd(gy, y, q, x, rsum, unorm, bsq, ws, gx, kind=KERNEL_GAUSSIAN):
    """Backward of that iteration (recomputes the kernel values): returns dL/dq, adds into ``gx``.  ``kind``:
    the kernel profile of the forward call."""
    require_cuda(gy, y, q, x, rsum, unorm, bsq, gx)
    x = _f32c(x, "x")
    B, N, D = x.shape
    gy, y, q = _f32c(gy, "gy"), _f32c(y, "y"), _f32c(q, "q")
    if not (tuple(gy.shape) == tuple(y.shape) == tuple(q.shape) == (B, N, D)):
        raise ValueError("meanshift_w_iter_bwd: gy, y, q must be (B,N,D) like x")
    rsum, unorm = _msw_rows(rsum, "rsum", B, N, x.device), _msw_rows(unorm, "unorm", B, N, x.device)
    bsq = _msw_bsq(bsq, B, x.device)
    if (ws.B, ws.N, ws.D, ws.backward) != (B, N, D, True) or tuple(gx.shape) != (B, N, D):
        raise ValueError("meanshift_w_iter_bwd: x, gx (B,N,D) and a backward workspace of that shape")
    if gx.dtype != torch.float32 or not gx.is_contiguous():
        raise TypeError("meanshift_w_iter_bwd: gx must be contiguous fp32")
    gq = torch.empty_like(x)
    with _lib.on_device(x.device):
        rc = _lib.load().pn_meanshift_w_iter_bwd_kind_f32(ptr(gy), ptr(y), ptr(q), ptr(x), ptr(rsum), ptr(unorm),
                                                          ptr(bsq), B, N, D, ptr(gq), ptr(gx), ptr(ws.buf),
                                                          ws.buf.numel(), int(ws.holds_image_of(x)), int(kind),
                                                          current_stream(x.device))
    check(rc, "pn_meanshift_w_iter_bwd_kind_f32")
    ws.took_image_of(x)
    return gq


def gemm_x3_weight_image(w, transposed=False):
    """Pre-split bf16 x 3 image of a weight w (M,K) for gemm_x3 (transposed: of w^T, for the gradient
    w.r.t. the activations).  Returns a uint8 tensor."""
    require_cuda(w)
    w = _f32c(w, "w")
    if w.dim() != 2:
        raise ValueError("gemm_x3_weight_image expects (M,K), got %s" % (tuple(w.shape),))
    M, Kd = w.shape
    lib = _lib.load()
    nbytes = lib.pn_gemm_x3_weight_image_bytes(Kd, M) if transposed else lib.pn_gemm_x3_weight_image_bytes(M, Kd)
    img = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
    with _lib.on_device(w.device):
        rc = lib.pn_gemm_x3_weight_image_f32(ptr(w), M, Kd, 1 if transposed else 0, ptr(img), current_stream(w.device))
    check(rc, "pn_gemm_x3_weight_image_f32")
    return img


def gemm_x3(img_a, M, x, bias=None):
    """out (B,M,N) = A x (+ bias): img_a = gemm_x3_weight_image of the (M,K) operand A, x (B,K,N) fp32
    channel-first.  fp32-grade products on the bf16 matrix cores (csrc/gemm_x3.hip)."""
    require_cuda(img_a, x)
    x = _f32c(x, "x")
    if x.dim() != 3:
        raise ValueError("gemm_x3 expects x (B,K,N), got %s" % (tuple(x.shape),))
    B, Kd, N = x.shape
    lib = _lib.load()
    if img_a.numel() != lib.pn_gemm_x3_weight_image_bytes(M, Kd):
        raise ValueError("gemm_x3: the weight image does not belong to a (%d,%d) operand" % (M, Kd))
    if bias is not None:
        bias = _f32c(bias, "bias")
        if bias.numel() != M:
            raise ValueError("gemm_x3: bias must have %d elements" % M)
    out = torch.empty((B, M, N), dtype=torch.float32, device=x.device)
    wsz = lib.pn_gemm_x3_points_image_bytes(B, Kd, N)
    ws = torch.empty(wsz, dtype=torch.uint8, device=x.device)
    with _lib.on_device(x.device):
        rc = lib.pn_gemm_x3_f32(ptr(img_a), ptr(x), ptr(bias), B, M, Kd, N, ptr(out), ptr(ws), wsz,
                                current_stream(x.device))
    check(rc, "pn_gemm_x3_f32")
    return out


def standardize_select(w, kf):
    """The confident points of S segments (src/fitting_utils.py:515-523): w (S,n) -> byte mask (S,n): w > 0.8, or
    the kf largest memberships of a row with fewer than 400 such points (ties to the smaller index)."""
    require_cuda(w)
    w = _f32c(w, "w")
    S, n = w.shape
    sel = torch.empty((S, n), dtype=torch.uint8, device=w.device)
    with _lib.on_device(w.device):
        rc = _lib.load().pn_standardize_select_f32(ptr(w), S, n, int(kf), ptr(sel), current_stream(w.device))
    check(rc, "pn_standardize_select_f32")
    return sel


def standardize_scale(Pr, w, sel, eps):
    """Pr (S,n,3) rotated centred points -> (pts (S,n,3) = Pr / (std + eps), std (S,3) = | max - min | of the
    weighted selected points per axis): src/fitting_utils.py:545-552."""
    Pr, w = _f32c(Pr, "Pr"), _f32c(w, "w")
    S, n, _ = Pr.shape
    pts = torch.empty_like(Pr)
    std = torch.empty((S, 3), dtype=torch.float32, device=Pr.device)
    with _lib.on_device(Pr.device):
        rc = _lib.load().pn_standardize_scale_f32(ptr(Pr), ptr(w), ptr(sel), S, n, float(eps), ptr(pts), ptr(std),
                                                  current_stream(Pr.device))
    check(rc, "pn_standardize_scale_f32")
    return pts, std


def gemm_x3_cat(img_a, M, xs, bias=None):
    """gemm_x3 applied to the concatenation of xs (a list of 1 to 4 tensors (B,C_s,N), every C_s a multiple of 8)
    along the channels — without writing the concatenation (src/model.py:150 builds it with torch.cat)."""
    import ctypes
    require_cuda(img_a, *xs)
    xs = [_f32c(t, "x") for t in xs]
    if not 1 <= len(xs) <= 4 or any(t.dim() != 3 or t.shape[0] != xs[0].shape[0] or t.shape[2] != xs[0].shape[2]
                                    or t.shape[1] % 8 for t in xs):
        raise ValueError("gemm_x3_cat expects 1 to 4 tensors (B,C_s,N) with C_s a multiple of 8")
    B, _, N = xs[0].shape
    Kd = sum(t.shape[1] for t in xs)
    lib = _lib.load()
    if img_a.numel() != lib.pn_gemm_x3_weight_image_bytes(M, Kd):
        raise ValueError("gemm_x3_cat: the weight image does not belong to a (%d,%d) operand" % (M, Kd))
    if bias is not None:
        bias = _f32c(bias, "bias")
    out = torch.empty((B, M, N), dtype=torch.float32, device=xs[0].device)
    wsz = lib.pn_gemm_x3_points_image_bytes(B, Kd, N)
    ws = torch.empty(wsz, dtype=torch.uint8, device=out.device)
    ptrs = (ctypes.c_void_p * len(xs))(*[t.data_ptr() for t in xs])
    chans = (ctypes.c_int * len(xs))(*[t.shape[1] for t in xs])
    with _lib.on_device(out.device):
        rc = lib.pn_gemm_x3_cat_f32(ptr(img_a), ptrs, chans, len(xs), ptr(bias), B, M, N, ptr(out), ptr(ws), wsz,
                                    current_stream(out.device))
    check(rc, "pn_gemm_x3_cat_f32")
    return out


def gemm_x3_wgrad(gy, x, want_bias=False):
    """Weight gradient of y[b] = W x[b] (+ bias): gw (M,K) = sum_b gy[b] x[b]^T over the points, bf16 x 3 on the
    matrix cores with a fixed-order split over the points (csrc/gemm_x3.hip).  gy (B,M,N), x (B,K,N) fp32
    channel-first.  Returns gw, or (gw, gb (M)) with ``want_bias``."""
    require_cuda(gy, x)
    gy, x = _f32c(gy, "gy"), _f32c(x, "x")
    if gy.dim() != 3 or x.dim() != 3 or gy.shape[0] != x.shape[0] or gy.shape[2] != x.shape[2]:
        raise ValueError("gemm_x3_wgrad expects gy (B,M,N) and x (B,K,N), got %s and %s"
                         % (tuple(gy.shape), tuple(x.shape)))
    B, M, N = gy.shape
    Kd = x.shape[1]
    lib = _lib.load()
    gw = torch.empty((M, Kd), dtype=torch.float32, device=x.device)
    gb = torch.empty((M,), dtype=torch.float32, device=x.device) if want_bias else None
    wsz = lib.pn_gemm_x3_wgrad_workspace(B, M, Kd, N)
    ws = torch.empty(wsz, dtype=torch.uint8, device=x.device)
    with _lib.on_device(x.device):
        rc = lib.pn_gemm_x3_wgrad_f32(ptr(gy), ptr(x), B, M, Kd, N, ptr(gw), ptr(gb), ptr(ws), wsz,
                                      current_stream(x.device))
    check(rc, "pn_gemm_x3_wgrad_f32")
    return (gw, gb) if want_bias else gw


def meanshift_rows_bwd(gy, y, q, rsum, unorm, x, bsq, gx, ws=None, kind=KERNEL_GAUSSIAN):
    """One step of the mean-shift backward restricted to R <= 64 rows per batch item (csrc/meanshift_rows.hip;
    src/mean_shift.py:45-79 maps every row on its own): gy, y, q (B,R,D), rsum, unorm (B,R), x (B,N,D),
    bsq (B); D = 32, 64 or 128.  Returns gq (B,R,D); ADDS the step's gradient w.r.t. the data into gx (B,N,D).
    ``kind``: the kernel profile of the forward pass (KERNEL_GAUSSIAN / KERNEL_EPANECHNIKOV)."""
    require_cuda(gy, y, q, rsum, unorm, x, bsq, gx)
    gy, y, q, x = _f32c(gy, "gy"), _f32c(y, "y"), _f32c(q, "q"), _f32c(x, "x")
    rsum, unorm, bsq = _f32c(rsum, "rsum"), _f32c(unorm, "unorm"), _f32c(bsq, "bsq")
    B, N, D = x.shape
    R = q.shape[1]
    if tuple(gy.shape) != (B, R, D) or tuple(y.shape) != (B, R, D) or tuple(q.shape) != (B, R, D):
        raise ValueError("meanshift_rows_bwd: gy, y, q must be (B,R,D)")
    if tuple(rsum.shape) != (B, R) or tuple(unorm.shape) != (B, R) or tuple(gx.shape) != (B, N, D):
        raise ValueError("meanshift_rows_bwd: rsum, unorm (B,R), gx (B,N,D)")
    if gx.dtype != torch.float32 or not gx.is_contiguous():
        raise TypeError("meanshift_rows_bwd: gx must be contiguous fp32")
    lib = _lib.load()
    wsz = lib.pn_meanshift_rows_bwd_workspace(B, N)
    if ws is None or ws.numel() < wsz:
        ws = torch.empty(wsz, dtype=torch.uint8, device=x.device)
    gq = torch.empty_like(q)
    with _lib.on_device(x.device):
        rc = lib.pn_meanshift_rows_bwd_kind_f32(ptr(gy), ptr(y), ptr(q), ptr(rsum), ptr(unorm), ptr(x), ptr(bsq), B, N,
                                                D, R, ptr(gq), ptr(gx), ptr(ws), ws.numel(), int(kind),
                                                current_stream(x.device))
    check(rc, "pn_meanshift_rows_bwd_kind_f32")
    return gq


def meanshift_rows_workspace(B, N, device):
    return torch.empty(_lib.load().pn_meanshift_rows_bwd_workspace(B, N), dtype=torch.uint8, device=device)


def meanshift_rows_scatter_add(gx, rows, g):
    """gx[b, rows[b,r], :] += g[b, r, :], r ascending, in place (rows (B,R) int64, repeats allowed)."""
    require_cuda(gx, rows, g)
    g = _f32c(g, "g")
    rows = _i64c(rows, "rows")
    B, N, D = gx.shape
    R = rows.shape[1]
    if tuple(g.shape) != (B, R, D) or gx.dtype != torch.float32 or not gx.is_contiguous():
        raise ValueError("meanshift_rows_scatter_add: g (B,R,D), gx contiguous fp32 (B,N,D)")
    with _lib.on_device(gx.device):
        rc = _lib.load().pn_meanshift_rows_scatter_add_f32(ptr(g), ptr(rows), B, N, D, R, ptr(gx),
                                                           current_stream(gx.device))
    check(rc, "pn_meanshift_rows_scatter_add_f32")
    return gx


def meanshift_h2_split(x):
    """x (B,N,128), unit rows -> pre-split fp16 x 2 tile images for the matrix-core path."""
    require_cuda(x)
    x = _f32c(x, "x")
    B, N, D = x.shape
    lib = _lib.load()
    img = torch.empty(lib.pn_meanshift_h2_image_bytes(B, N), dtype=torch.uint8, device=x.device)
    with _lib.on_device(x.device):
        rc = lib.pn_meanshift_h2_split_f32(ptr(x), B, N, D, ptr(img), current_stream(x.device))
    check(rc, "pn_meanshift_h2_split_f32")
    return img


def meanshift_h2_iter_fwd(q, x_image, bsq, ws):
    B, N, D = q.shape
    y, rsum, unorm = _ms_out("meanshift_h2_iter_fwd", q, None)
    with _lib.on_device(q.device):
        rc = _lib.load().pn_meanshift_h2_iter_fwd_f32(ptr(q), ptr(x_image), ptr(bsq), B, N, D, ptr(ws.opart),
                                                      ptr(ws.rpart), ptr(y), ptr(rsum), ptr(unorm),
                                                      current_stream(q.device))
    check(rc, "pn_meanshift_h2_iter_fwd_f32")
    return y, rsum, unorm


def meanshift_h2_iter_bwd(gy, y, q, x, x_image, rsum, unorm, bsq, ws, gx):
    """fp16 x 2 counterpart of meanshift_iter_bwd: returns dL/dq, adds into ``gx``."""
    B, N, D = x.shape
    gy = _f32c(gy, "gy")
    gq = torch.empty_like(x)
    lib = _lib.load()
    if ws.h2_imgs is None:
        nbytes = lib.pn_meanshift_h2_image_bytes(B, N)
        ws.h2_imgs = [torch.empty(nbytes, dtype=torch.uint8, device=x.device) for _ in range(2)]
    im = ws.h2_imgs
    with _lib.on_device(x.device):
        rc = lib.pn_meanshift_h2_iter_bwd_f32(ptr(gy), ptr(y), ptr(q), ptr(x), ptr(x_image), ptr(rsum),
                                              ptr(unorm), ptr(bsq), B, N, D, ptr(ws.gu), ptr(ws.cs), ptr(im[0]),
                                              ptr(im[1]), ptr(ws.opart), ptr(ws.opart_x), ptr(gq), ptr(gx),
                                              current_stream(x.device))
    check(rc, "pn_meanshift_h2_iter_bwd_f32")
    return gq


def meanshift_iter_fwd(q, x, xt, bsq, ws):
    B, N, D = x.shape
    y, rsum, unorm = _ms_out("meanshift_iter_fwd", x, None)
    with _lib.on_device(x.device):
        rc = _lib.load().pn_meanshift_iter_fwd_f32(ptr(q), ptr(x), ptr(xt), ptr(bsq), B, N, D, ptr(ws.opart),
                                                   ptr(ws.rpart), ptr(y), ptr(rsum), ptr(unorm),
                                                   current_stream(x.device))
    check(rc, "pn_meanshift_iter_fwd_f32")
    return y, rsum, unorm


def meanshift_iter_bwd(gy, y, q, x, xt, rsum, unorm, bsq, ws, gx):
    """Returns dL/dq (B,N,D) and adds this iteration's contribution to dL/dx into ``gx``."""
    B, N, D = x.shape
    gy = _f32c(gy, "gy")
    gq = torch.empty_like(x)
    with _lib.on_device(x.device):
        rc = _lib.load().pn_meanshift_iter_bwd_f32(ptr(gy), ptr(y), ptr(q), ptr(x), ptr(xt), ptr(rsum),
                                                   ptr(unorm), ptr(bsq), B, N, D, ptr(ws.gu), ptr(ws.go),
                                                   ptr(ws.cs), ptr(ws.qt), ptr(ws.gut), ptr(ws.opart),
                                                   ptr(ws.opart_x), ptr(gq), ptr(gx),
                                                   current_stream(x.device))
    check(rc, "pn_meanshift_iter_bwd_f32")
    return gq


def sym3_eig(G):
    """G (M,3,3) float64 symmetric -> (evals (M,3) descending, evecs (M,3,3), columns)."""
    require_cuda(G)
    if G.dtype != torch.float64:
        raise TypeError("sym3_eig expects float64")
    G = G.contiguous()
    M = G.shape[0]
    evals = torch.empty((M, 3), dtype=torch.float64, device=G.device)
    evecs = torch.empty((M, 3, 3), dtype=torch.float64, device=G.device)
    with _lib.on_device(G.device):
        rc = _lib.load().pn_sym3_eig_f64(ptr(G), M, ptr(evals), ptr(evecs), current_stream(G.device))
    check(rc, "pn_sym3_eig_f64")
    return evals, evecs


def _i32c(t, name):
    if t.dtype != torch.int32:
        raise TypeError("%s must be int32, got %s" % (name, t.dtype))
    return t.contiguous()


def chamfer_nn_ragged(a, off_a, max_a, b, off_b, max_b, side_a=True, side_b=True):
    """Ragged batch of nearest-neighbour searches: item i is a[off_a[i]:off_a[i+1]] against
    b[off_b[i]:off_b[i+1]] (a (TA,3), b (TB,3) fp32; offsets (B+1,) int32 on the GPU; max_* the
    largest item sizes, known to the host).  Returns (minA (TA,), argA (TA,), minB (TB,), argB (TB,))
    with indices local to the item; sides not requested are None."""
    require_cuda(a, b, off_a, off_b)
    a = _f32c(a, "a")
    b = _f32c(b, "b")
    off_a, off_b = _i32c(off_a, "off_a"), _i32c(off_b, "off_b")
    TA, TB = a.shape[0], b.shape[0]
    B = off_a.shape[0] - 1
    if B < 1 or off_b.shape[0] != B + 1 or TA == 0 or TB == 0:
        raise ValueError("chamfer_nn_ragged: empty batch")
    lib = _lib.load()
    dev = a.device
    minA = argA = minB = argB = None
    if side_a:
        minA = torch.empty(TA, dtype=torch.float32, device=dev)
        argA = torch.empty(TA, dtype=torch.int64, device=dev)
    if side_b:
        minB = torch.empty(TB, dtype=torch.float32, device=dev)
        argB = torch.empty(TB, dtype=torch.int64, device=dev)
    wsz = lib.pn_chamfer_nn_ragged_workspace(TA, TB)
    ws = torch.empty(wsz, dtype=torch.uint8, device=dev)
    with _lib.on_device(dev):
        rc = lib.pn_chamfer_nn_ragged_f32(ptr(a), ptr(off_a), TA, int(max_a), ptr(b), ptr(off_b), TB, int(max_b),
                                          B, ptr(minA), ptr(argA), ptr(minB), ptr(argB), ptr(ws), wsz,
                                          current_stream(dev))
    check(rc, "pn_chamfer_nn_ragged_f32")
    return minA, argA, minB, argB


def chamfer_ragged_reduce(minA, off_a, minB, off_b):
    """(mean minA + mean minB) / 2 per item of the ragged batch, fixed summation order -> (S,)."""
    require_cuda(minA, minB)
    S = off_a.shape[0] - 1
    out = torch.empty(S, dtype=torch.float32, device=minA.device)
    with _lib.on_device(minA.device):
        rc = _lib.load().pn_chamfer_ragged_reduce_f32(ptr(_f32c(minA, "minA")), ptr(_i32c(off_a, "off_a")),
                                                      ptr(_f32c(minB, "minB")), ptr(_i32c(off_b, "off_b")), S,
                                                      ptr(out), current_stream(minA.device))
    check(rc, "pn_chamfer_ragged_reduce_f32")
    return out


def coverage_reduce(minA, off_a, minB, off_b):
    """The coverage figures of S shapes from the SQUARED nearest-neighbour minima of both sides (ragged, offsets (S+1,)
    int32 on the GPU) -> (S,6) float64 on the GPU: per side the fp64 sum of sqrt(clamp(x, 1e-5)) (fp32 roots), the
    count of roots < 0.01 and the count < 0.02 (fp32 comparisons).  Fixed summation order, no atomics: a shape's row
    does not depend on the batch around it."""
    require_cuda(minA, minB, off_a, off_b)
    off_a, off_b = _i32c(off_a, "off_a"), _i32c(off_b, "off_b")
    S = off_a.shape[0] - 1
    if S < 1 or off_b.shape[0] != S + 1:
        raise ValueError("coverage_reduce: offsets of %d and %d entries" % (off_a.shape[0], off_b.shape[0]))
    out = torch.empty((S, 6), dtype=torch.float64, device=minA.device)
    with _lib.on_device(minA.device):
        rc = _lib.load().pn_coverage_reduce_f32(ptr(_f32c(minA, "minA")), ptr(off_a), ptr(_f32c(minB, "minB")),
                                                ptr(off_b), S, ptr(out), current_stream(minA.device))
    check(rc, "pn_coverage_reduce_f32")
    return out


def chamfer_ragged_bwd(pred, off_a, max_a, gt, off_b, argA, argB, g):
    """Gradient of chamfer_ragged_reduce with respect to the predictions (TA,3); g (S,)."""
    require_cuda(pred, gt, g)
    pred, gt, g = _f32c(pred, "pred"), _f32c(gt, "gt"), _f32c(g, "g")
    S = off_a.shape[0] - 1
    gpred = torch.empty_like(pred)
    with _lib.on_device(pred.device):
        rc = _lib.load().pn_chamfer_ragged_bwd_f32(ptr(pred), ptr(_i32c(off_a, "off_a")), int(max_a), ptr(gt),
                                                   ptr(_i32c(off_b, "off_b")), ptr(_i64c(argA, "argA")),
                                                   ptr(_i64c(argB, "argB")), ptr(g), S, ptr(gpred),
                                                   current_stream(pred.device))
    check(rc, "pn_chamfer_ragged_bwd_f32")
    return gpred


def gather_rows3_bwd(g, idx, N):
    """g (B,M,3), idx (B,M) int64 -> (B,N,3): rows of g added into the rows idx names, ascending m."""
    require_cuda(g, idx)
    g, idx = _f32c(g, "g"), _i64c(idx, "idx")
    B, M, _ = g.shape
    out = torch.empty((B, N, 3), dtype=torch.float32, device=g.device)
    with _lib.on_device(g.device):
        rc = _lib.load().pn_gather_rows3_bwd_f32(ptr(g), ptr(idx), B, M, N, ptr(out), current_stream(g.device))
    check(rc, "pn_gather_rows3_bwd_f32")
    return out


# ---- batched primitive fits (csrc/fitbatch.hip) ---------------------------------------------
PRIM_PLANE, PRIM_SPHERE, PRIM_CYLINDER, PRIM_CONE = 0, 1, 2, 3
FIT_NPAR = 16


def weighted_moments(P, Nrm, W, seg_shape, seg_row, stride, eps):
    """P, Nrm (B,N,3), W (B,Cp,N) fp32; seg_* (S,) int32 -> partial moment sums (S, chunks, 64) fp64."""
    require_cuda(P, Nrm, W, seg_shape, seg_row)
    P, Nrm, W = _f32c(P, "P"), _f32c(Nrm, "Nrm"), _f32c(W, "W")
    B, N, _ = P.shape
    Cp = W.shape[1]
    S = seg_shape.shape[0]
    lib = _lib.load()
    partial = torch.empty((S, lib.pn_weighted_moments_chunks(), lib.pn_weighted_moments_count()),
                          dtype=torch.float64, device=P.device)
    with _lib.on_device(P.device):
        rc = lib.pn_weighted_moments_f64(ptr(P), ptr(Nrm), ptr(W), B, N, Cp, int(stride), float(eps),
                                         ptr(_i32c(seg_shape, "seg_shape")), ptr(_i32c(seg_row, "seg_row")), S,
                                         ptr(partial), current_stream(P.device))
    check(rc, "pn_weighted_moments_f64")
    return partial


def primitive_fit(partial, seg_type, seg_rows):
    """partial (S,chunks,64) fp64 -> params (S,16) fp64, jac (S,16,64) fp64, status (S,) int32."""
    require_cuda(partial, seg_type, seg_rows)
    S = partial.shape[0]
    dev = partial.device
    params = torch.empty((S, FIT_NPAR), dtype=torch.float64, device=dev)
    jac = torch.empty((S, FIT_NPAR, partial.shape[2]), dtype=torch.float64, device=dev)
    status = torch.empty(S, dtype=torch.int32, device=dev)
    with _lib.on_device(dev):
        rc = _lib.load().pn_primitive_fit_f64(ptr(partial.contiguous()), ptr(_i32c(seg_type, "seg_type")),
                                              ptr(_i32c(seg_rows, "seg_rows")), S, ptr(params), ptr(jac),
                                              ptr(status), current_stream(dev))
    check(rc, "pn_primitive_fit_f64")
    return params, jac, status


def cone_angle(P, W, seg_shape, seg_row, seg_type, status, params, jac, stride, eps):
    """Second pass of the cone fit; updates params[:,6] and jac[:,6,:] in place, returns cone_direct (S,)."""
    require_cuda(P, W, params, jac)
    P, W = _f32c(P, "P"), _f32c(W, "W")
    B, N, _ = P.shape
    S = seg_shape.shape[0]
    cone_direct = torch.empty(S, dtype=torch.float64, device=P.device)
    with _lib.on_device(P.device):
        rc = _lib.load().pn_cone_angle_f64(ptr(P), ptr(W), B, N, W.shape[1], int(stride), float(eps),
                                           ptr(seg_shape), ptr(seg_row), ptr(seg_type), ptr(status), S,
                                           ptr(params), ptr(jac), ptr(cone_direct), current_stream(P.device))
    check(rc, "pn_cone_angle_f64")
    return cone_direct


def primitive_residual(P, seg_shape, seg_type, gt_off, gt_idx, params, status, sqrt_flag=False):
    """Mean residual of the ground-truth points of every segment: dist (S,) fp32, dparam (S,16) fp64."""
    require_cuda(P, gt_off, gt_idx, params)
    B, N, _ = P.shape
    S = seg_shape.shape[0]
    dist = torch.empty(S, dtype=torch.float32, device=P.device)
    dparam = torch.zeros((S, FIT_NPAR), dtype=torch.float64, device=P.device)
    with _lib.on_device(P.device):
        rc = _lib.load().pn_primitive_residual_f32(ptr(_f32c(P, "P")), B, N, ptr(seg_shape), ptr(seg_type),
                                                   ptr(_i32c(gt_off, "gt_off")), ptr(_i32c(gt_idx, "gt_idx")), S,
                                                   ptr(params), int(bool(sqrt_flag)), ptr(dist), ptr(dparam),
                                                   ptr(status), current_stream(P.device))
    check(rc, "pn_primitive_residual_f32")
    return dist, dparam


def weighted_moments_bwd(P, Nrm, W, seg_shape, seg_row, seg_type, g_dist, dparam, jac, params, cone_direct,
                         stride, eps):
    """d loss / d W (B,Cp,N) fp32 of the batched fits given g_dist (S,) = d loss / d dist."""
    require_cuda(P, Nrm, W, g_dist)
    P, Nrm, W = _f32c(P, "P"), _f32c(Nrm, "Nrm"), _f32c(W, "W")
    B, N, _ = P.shape
    S = seg_shape.shape[0]
    gW = torch.zeros_like(W)
    with _lib.on_device(P.device):
        rc = _lib.load().pn_weighted_moments_bwd_f32(ptr(P), ptr(Nrm), ptr(W), B, N, W.shape[1], int(stride),
                                                     float(eps), ptr(seg_shape), ptr(seg_row), ptr(seg_type), S,
                                                     ptr(_f32c(g_dist, "g_dist")), ptr(dparam), ptr(jac),
                                                     ptr(params), ptr(cone_direct), ptr(gW),
                                                     current_stream(P.device))
    check(rc, "pn_weighted_moments_bwd_f32")
    return gW


def bspline_eval(nu, nv, ctrl, affine=None, wrap=False):
    """ctrl (S,cu,cv,3), nu (gu,cu), nv (gv,cv) fp32 -> (S,(gu+wrap)*gv,3); affine (S,3,4) optional."""
    require_cuda(nu, nv, ctrl, affine)
    nu, nv, ctrl = _f32c(nu, "nu"), _f32c(nv, "nv"), _f32c(ctrl, "ctrl")
    S, cu, cv, _ = ctrl.shape
    gu, gv = nu.shape[0], nv.shape[0]
    if affine is not None:
        affine = _f32c(affine, "affine")
    out = torch.empty((S, (gu + int(wrap)) * gv, 3), dtype=torch.float32, device=ctrl.device)
    with _lib.on_device(ctrl.device):
        rc = _lib.load().pn_bspline_eval_f32(ptr(nu), ptr(nv), ptr(ctrl), ptr(affine), S, gu, gv, cu, cv, int(wrap),
                                             ptr(out), current_stream(ctrl.device))
    check(rc, "pn_bspline_eval_f32")
    return out


def bspline_eval_bwd(nu, nv, gout, affine, cu, cv, wrap=False):
    require_cuda(nu, nv, gout, affine)
    nu, nv, gout = _f32c(nu, "nu"), _f32c(nv, "nv"), _f32c(gout, "gout")
    S = gout.shape[0]
    gu, gv = nu.shape[0], nv.shape[0]
    if affine is not None:
        affine = _f32c(affine, "affine")
    gctrl = torch.empty((S, cu, cv, 3), dtype=torch.float32, device=gout.device)
    with _lib.on_device(gout.device):
        rc = _lib.load().pn_bspline_eval_bwd_f32(ptr(nu), ptr(nv), ptr(gout), ptr(affine), S, gu, gv, cu, cv,
                                                 int(wrap), ptr(gctrl), current_stream(gout.device))
    check(rc, "pn_bspline_eval_bwd_f32")
    return gctrl


# ---- round-3 fusions (csrc/fused.hip) ----------------------------------------------------------
def edgeconv_bwd_stats(gout, yext, mean, rstd, gamma, beta, groups, per_sample, dense, slope, k):
    """Step A of the fused edge-conv backward with its reductions: returns (t (B,N,Cout), dgamma,
    dbeta (Cout), c1c2 ((B or 1), groups, 2))."""
    require_cuda(gout, yext)
    gout = _f32c(gout, "gout")
    B, N, Cout = yext.shape
    dev = yext.device
    t = torch.empty_like(yext)
    dgamma = torch.empty(Cout, dtype=torch.float32, device=dev)
    dbeta = torch.empty(Cout, dtype=torch.float32, device=dev)
    c1c2 = torch.empty((B if per_sample else 1, groups, 2), dtype=torch.float32, device=dev)
    lib = _lib.load()
    wsz = lib.pn_edgeconv_bwd_stats_workspace(B, N, Cout)
    ws = torch.empty(wsz, dtype=torch.uint8, device=dev)
    with _lib.on_device(dev):
        rc = lib.pn_edgeconv_bwd_stats_f32(ptr(gout), ptr(yext), ptr(mean), ptr(rstd), ptr(_f32c(gamma, "gamma")),
                                           ptr(_f32c(beta, "beta")), B, N, int(k), Cout, int(groups),
                                           int(per_sample), int(dense), float(slope), ptr(t), ptr(dgamma),
                                           ptr(dbeta), ptr(c1c2), ptr(ws), wsz, current_stream(dev))
    check(rc, "pn_edgeconv_bwd_stats_f32")
    return t, dgamma, dbeta, c1c2


def triplet_fwd(E, ia, ib, w, margin):
    """E (rows,D) fp32, D = 32, 64 or 128; ia, ib (P,num) int64 row indices; w (P,) fp32 -> (loss (1,), item_scale (P,))."""
    require_cuda(E, ia, ib, w)
    E = _f32c(E, "E")
    ia, ib = _i64c(ia, "ia"), _i64c(ib, "ib")
    P, num = ia.shape
    dev = E.device
    item_loss = torch.empty(P, dtype=torch.float32, device=dev)
    item_scale = torch.empty(P, dtype=torch.float32, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    with _lib.on_device(dev):
        rc = _lib.load().pn_triplet_fwd_f32(ptr(E), E.shape[0], E.shape[1], ptr(ia), ptr(ib), ptr(_f32c(w, "w")), P,
                                            num, float(margin), ptr(item_loss), ptr(item_scale), ptr(loss),
                                            current_stream(dev))
    check(rc, "pn_triplet_fwd_f32")
    return loss, item_scale


def triplet_bwd(E, ia, ib, item_scale, gout, margin):
    """d loss / d E (rows,D) scaled by gout (1,)."""
    require_cuda(E, gout)
    P, num = ia.shape
    gE = torch.zeros_like(E)
    lib = _lib.load()
    wsz = lib.pn_triplet_bwd_workspace(P, num, E.shape[1])
    ws = torch.empty(wsz, dtype=torch.uint8, device=E.device)
    with _lib.on_device(E.device):
        rc = lib.pn_triplet_bwd_f32(ptr(E), E.shape[0], E.shape[1], ptr(ia), ptr(ib), ptr(item_scale),
                                    ptr(_f32c(gout.reshape(1), "gout")), P, num, float(margin), ptr(gE),
                                    ptr(ws), wsz, current_stream(E.device))
    check(rc, "pn_triplet_bwd_f32")
    return gE


def membership_fwd(cen, emb, bw, ncl, eps, want_labels=False):
    """cen (B,CP,D), emb (B,N,D), D = 32, 64 or 128, bw (B,), ncl (B,) int64 -> Wraw, prob, Wn (B,CP,N), rowstat (B,CP,4),
    labels (B,N) int64 or None."""
    require_cuda(cen, emb, bw, ncl)
    cen, emb, bw = _f32c(cen, "cen"), _f32c(emb, "emb"), _f32c(bw, "bw")
    ncl = _i64c(ncl, "ncl")
    B, CP, D = cen.shape
    N = emb.shape[1]
    dev = emb.device
    Wraw = torch.empty((B, CP, N), dtype=torch.float32, device=dev)
    prob = torch.empty_like(Wraw)
    Wn = torch.empty_like(Wraw)
    rowstat = torch.empty((B, CP, 4), dtype=torch.float32, device=dev)
    labels = torch.empty((B, N), dtype=torch.int64, device=dev) if want_labels else None
    with _lib.on_device(dev):
        rc = _lib.load().pn_membership_fwd_f32(ptr(cen), ptr(emb), ptr(bw), ptr(ncl), B, CP, N, D, float(eps),
                                               ptr(Wraw), ptr(prob), ptr(Wn), ptr(rowstat), ptr(labels),
                                               current_stream(dev))
    check(rc, "pn_membership_fwd_f32")
    return Wraw, prob, Wn, rowstat, labels


def membership_bwd(gWn, Wraw, prob, rowstat, bw, ncl):
    require_cuda(gWn, Wraw)
    gWn = _f32c(gWn, "gWn")
    B, CP, N = Wraw.shape
    rowgrad = torch.empty((B, CP, 2), dtype=torch.float32, device=Wraw.device)
    gWraw = torch.empty_like(Wraw)
    with _lib.on_device(Wraw.device):
        rc = _lib.load().pn_membership_bwd_f32(ptr(gWn), ptr(Wraw), ptr(prob), ptr(rowstat), ptr(bw), ptr(ncl), B, CP,
                                               N, ptr(rowgrad), ptr(gWraw), current_stream(Wraw.device))
    check(rc, "pn_membership_bwd_f32")
    return gWraw


def affine_act_fwd(x, scale, shift, act, slope=0.0):
    """act(x * scale[c] + shift[c]) on (B,C,N); act 0 none, 1 ReLU, 2 LeakyReLU(slope)."""
    require_cuda(x, scale, shift)
    x = _f32c(x, "x")
    B, C, N = x.shape
    y = torch.empty_like(x)
    with _lib.on_device(x.device):
        rc = _lib.load().pn_affine_act_fwd_f32(ptr(x), ptr(_f32c(scale, "scale")), ptr(_f32c(shift, "shift")), B, C, N,
                                               int(act), float(slope), ptr(y), current_stream(x.device))
    check(rc, "pn_affine_act_fwd_f32")
    return y


def affine_act_bwd(gy, y, scale, act, slope=0.0):
    gy = _f32c(gy, "gy")
    B, C, N = y.shape
    gx = torch.empty_like(y)
    with _lib.on_device(y.device):
        rc = _lib.load().pn_affine_act_bwd_f32(ptr(gy), ptr(y), ptr(_f32c(scale, "scale")), B, C, N, int(act),
                                               float(slope), ptr(gx), current_stream(y.device))
    check(rc, "pn_affine_act_bwd_f32")
    return gx


def nms_occupied(membership, U):
    """membership (B,N) int64 -> (counts (B,N) int32, uq (B,U) int64 ascending occupied centres, nocc (B,) int64)."""
    require_cuda(membership)
    membership = _i64c(membership, "membership")
    B, N = membership.shape
    dev = membership.device
    counts = torch.empty((B, N), dtype=torch.int32, device=dev)
    uq = torch.empty((B, U), dtype=torch.int64, device=dev)
    nocc = torch.empty(B, dtype=torch.int64, device=dev)
    with _lib.on_device(dev):
        rc = _lib.load().pn_nms_occupied_f32(ptr(membership), B, N, int(U), ptr(counts), ptr(uq), ptr(nocc),
                                             current_stream(dev))
    check(rc, "pn_nms_occupied_f32")
    return counts, uq, nocc


def nms_vote(G, uq, nocc, counts, bw, cmax):
    """G (B,U,U) Gram matrix of the occupied centres -> (cid (B,cmax) int64 ascending voted centres, ncl (B,))."""
    require_cuda(G, uq, nocc, counts, bw)
    G = _f32c(G, "G")
    B, U, _ = G.shape
    N = counts.shape[1]
    dev = G.device
    hits = torch.empty((B, N), dtype=torch.int32, device=dev)
    cid = torch.empty((B, cmax), dtype=torch.int64, device=dev)
    ncl = torch.empty(B, dtype=torch.int64, device=dev)
    with _lib.on_device(dev):
        rc = _lib.load().pn_nms_vote_f32(ptr(G), ptr(uq), ptr(nocc), ptr(counts), ptr(_f32c(bw, "bw")), B, N, U,
                                         int(cmax), ptr(hits), ptr(cid), ptr(ncl), current_stream(dev))
    check(rc, "pn_nms_vote_f32")
    return cid, ncl


def weighted_max_fwd(x, scale, shift, w, act, slope=0.0):
    """max over n of act(x * scale[c] + shift[c]) * w[s, n]: x (S,C,N), w (S,N) -> (out (S,C), idx int32, val)."""
    require_cuda(x, scale, shift, w)
    x, w = _f32c(x, "x"), _f32c(w, "w")
    S, C, N = x.shape
    dev = x.device
    out = torch.empty((S, C), dtype=torch.float32, device=dev)
    idx = torch.empty((S, C), dtype=torch.int32, device=dev)
    val = torch.empty((S, C), dtype=torch.float32, device=dev)
    with _lib.on_device(dev):
        rc = _lib.load().pn_weighted_max_fwd_f32(ptr(x), ptr(_f32c(scale, "scale")), ptr(_f32c(shift, "shift")), ptr(w),
                                                 S, C, N, int(act), float(slope), ptr(out), ptr(idx), ptr(val),
                                                 current_stream(dev))
    check(rc, "pn_weighted_max_fwd_f32")
    return out, idx, val


def weighted_max_bwd(g, idx, val, N):
    g = _f32c(g, "g")
    S, C = g.shape
    gw = torch.empty((S, N), dtype=torch.float32, device=g.device)
    with _lib.on_device(g.device):
        rc = _lib.load().pn_weighted_max_bwd_f32(ptr(g), ptr(idx), ptr(val), S, C, int(N), ptr(gw),
                                                 current_stream(g.device))
    check(rc, "pn_weighted_max_bwd_f32")
    return gw


COVER_SAMPLED = 4   # type ids of pn_point_primitive_min_f32: 0 plane, 1 sphere, 2 cylinder, 3 cone, 4 sampled


def point_primitive_min(points, pt_off, prim_off, prim_type, prim_par, samp, samp_off):
    """Distance of every point to the nearest primitive of its shape (csrc/cover.hip), B shapes in ONE launch.
    points (T,3), prim_par (S,16), samp (C,3) or None: fp32 on the GPU.  pt_off (B+1), prim_off (B+1), prim_type (S),
    samp_off (S+1): HOST integer arrays — they are checked here (ascending, inside the arrays they index, a sampled
    primitive has at least one sample) and uploaded with the tile table in one copy.
    Returns (dmin (T) fp32, arg (T) int32: index within the shape, lowest on ties; -1 for a shape without primitives)."""
    import numpy as np
    require_cuda(points, prim_par, samp)
    points, prim_par = _f32c(points, "points"), _f32c(prim_par, "prim_par")
    pt_off, prim_off, prim_type, samp_off = [np.asarray(a, np.int64).reshape(-1)
                                             for a in (pt_off, prim_off, prim_type, samp_off)]
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("point_primitive_min expects (T,3) points, got %s" % (tuple(points.shape),))
    T, S, B = points.shape[0], prim_type.shape[0], pt_off.shape[0] - 1
    C = 0
    if samp is not None:
        samp = _f32c(samp, "samp")
        if samp.dim() != 2 or samp.shape[1] != 3:
            raise ValueError("point_primitive_min expects (C,3) samples, got %s" % (tuple(samp.shape),))
        C = samp.shape[0]
    if B < 1 or T < 1 or S < 1 or prim_off.shape[0] != B + 1 or samp_off.shape[0] != S + 1 or tuple(prim_par.shape) != (S, FIT_NPAR):
        raise ValueError("point_primitive_min: tables of %d shapes, %d points and %d primitives do not fit together"
                         % (B, T, S))
    for name, off, end in (("pt_off", pt_off, T), ("prim_off", prim_off, S), ("samp_off", samp_off, C)):
        if off[0] != 0 or off[-1] != end or (np.diff(off) < 0).any():
            raise ValueError("point_primitive_min: %s must ascend from 0 to %d" % (name, end))
    if (prim_type < 0).any() or (prim_type > COVER_SAMPLED).any():
        raise ValueError("point_primitive_min: type ids are 0 .. %d" % COVER_SAMPLED)
    if (np.diff(samp_off)[prim_type == COVER_SAMPLED] < 1).any():
        raise ValueError("point_primitive_min: a sampled primitive without samples")
    if max(T, C) * 3 >= 2 ** 31:
        raise ValueError("point_primitive_min: int32 offsets")
    lib = _lib.load()
    dev = points.device
    tile = lib.pn_point_primitive_min_tile()
    n = np.diff(pt_off)
    tiles = (n + tile - 1) // tile
    tile_shape = np.repeat(np.arange(B), tiles)
    tile_first = pt_off[tile_shape] + (np.arange(int(tiles.sum())) - np.repeat(np.cumsum(tiles) - tiles, tiles)) * tile
    table = _lib.h2d(np.concatenate([pt_off, prim_off, prim_type, samp_off, tile_shape, tile_first]).astype(np.int32), dev)
    o = np.cumsum([0, B + 1, B + 1, S, S + 1, tile_shape.shape[0]])
    col = [table[o[i]:o[i + 1] if i + 1 < len(o) else None] for i in range(len(o))]
    dmin = torch.empty(T, dtype=torch.float32, device=dev)
    arg = torch.empty(T, dtype=torch.int32, device=dev)
    with _lib.on_device(dev):
        rc = lib.pn_point_primitive_min_f32(ptr(points), ptr(col[0]), ptr(col[1]), ptr(col[2]), ptr(prim_par), ptr(samp),
                                            ptr(col[3]), ptr(col[4]), ptr(col[5]), B, int(tile_shape.shape[0]),
                                            ptr(dmin), ptr(arg), current_stream(dev))
    check(rc, "pn_point_primitive_min_f32")
    return dmin, arg
