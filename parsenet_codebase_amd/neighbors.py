"""Nearest neighbours ACROSS two clouds of any size, and k-nearest-sample lifting on them.

``nearest`` answers "which points of the reference are nearest to these points" for a scan against a scan, a scan
against the samples of its reconstruction, or the points of a scan against the samples the network saw — exactly, on a
uniform grid built over the reference (csrc/knn3_query.hip), at any size.  ``cloud_distance`` is its k = 1 distance: the
deviation map of one cloud against another.  ``lift_knn`` carries per-sample values back to every point through the k
nearest samples, with inverse-distance weights (floating values; PointNet++'s three_nn / three_interpolate for any k)
or a majority vote (integer labels): the way back from the network when ``sampling.lift``'s one nearest sample is too
coarse — stair-steps along segment boundaries — or when the points never went through ``reduce_cloud`` and have no
``owner``: a second scan of the same part, the points ``remove_outliers`` dropped, a denser re-scan.

    reduced, owner = reduce_cloud(scan, 10000)                 # before the network
    labels_full = lift_knn(labels_of_reduced, scan, reduced)   # after it: majority of the 3 nearest samples
    rows_full = lift_knn(membership_rows, other_scan, reduced) # smooth, and for points that were never reduced

Every function takes (N,3), (B,N,3) or a list of (N_b,3) fp32 clouds on the GPU; ``points`` and ``reference`` may
differ in layout and sizes but must hold the same number of clouds: cloud s of the points is searched in cloud s of the
reference.  All results are functions of the inputs alone, the same bits from run to run and for every batching, and no
function synchronises with the host.

Limits.  The weights follow the Euclidean distance, so a thin wall is still crossed: a point takes from samples on the
other side when they are nearer.  The grid follows the reference's bounding CUBE with at most n/4 cells: a reference
crowded into one corner of its box costs the queries in the empty part many rings (slow, never wrong)."""
import numbers

import torch

from . import kernels as K
from .ragged import Clouds


def _pair(who, points, reference):
    p = Clouds(points, who, bad_dtype=TypeError)
    r = Clouds(reference, who, bad_dtype=TypeError)
    if p.S != r.S:
        raise ValueError("%s: %d clouds of points against %d reference clouds" % (who, p.S, r.S))
    if p.flat.device != r.flat.device:
        raise ValueError("%s: the points are on %s, the reference on %s" % (who, p.flat.device, r.flat.device))
    return p, r


def _k(who, k):
    if isinstance(k, bool) or not isinstance(k, numbers.Integral):
        raise TypeError("%s: k must be an integer, got %r" % (who, k))
    if not K.QUERY_MIN_K <= k <= K.QUERY_MAX_K:
        raise ValueError("%s: k must be %d .. %d, got %d" % (who, K.QUERY_MIN_K, K.QUERY_MAX_K, k))
    return k


def nearest(points, reference, k=1, return_dist=False):
    """The k nearest reference points of every point.  Returns idx, int64 indices into the point's reference cloud,
    (N,k), (B,N,k) or a list of (N_b,k) in the layout of ``points`` — nearest first under the fp32
    ((dx² + dy²) + dz²), equal distances to the smaller index — and, with ``return_dist``, their fp32 distances.

    A reference cloud of n_r < k points fills the row from n_r on with idx -1 and distance +inf (an empty reference:
    every entry).  A reference cloud that holds a non-finite coordinate gives every row of its points idx -1 and
    distance NaN; a point with a non-finite coordinate gives that row alone idx -1, NaN.  CAUTION: ``reference[idx]``
    on a -1 gathers the LAST row of the reference, the wrong one, without an error — mask with ``idx >= 0`` first.
    1 <= k <= 64, N k < 2^31.  Exact, O((n_r + N) k); eight stream-ordered launches, no host synchronisation."""
    k = _k("nearest", k)
    p, r = _pair("nearest", points, reference)
    out = K.knn3_query(r.flat, r, p.flat, p, k, want_dist=return_dist)
    if return_dist:
        return p.per_point(out[0].long()), p.per_point(out[1])
    return p.per_point(out.long())


def cloud_distance(points, reference):
    """The distance of every point to its nearest reference point, fp32, (N,), (B,N) or a list of (N_b,): the
    deviation map of one scan against another, or against a reconstruction's samples, at any size.  +inf against an
    empty reference, NaN as ``nearest`` defines it.

    This is always the grid search.  Where the brute-force ``kernels.chamfer_nn_ragged`` is faster (small clouds:
    profiles/knn3_query.txt has the sizes) this function does NOT switch engines: one definition, one kernel."""
    p, r = _pair("cloud_distance", points, reference)
    _, dist = K.knn3_query(r.flat, r, p.flat, p, 1, want_dist=True)
    return p.per_point(dist[:, 0])


def lift_knn(values, points, samples, k=3):
    """Per-sample ``values`` carried to every point through its k nearest ``samples``.

    values: one row per sample, in the layout of ``samples`` — (m,...), (B,m,...) or a list of (m_b,...).
      floating (fp32, any trailing shape, flattened to C channels): inverse-distance interpolation,
        w_j = 1 / ((double) dist_j + 1e-8), out = (float)(Σ w_j v_j / Σ w_j) in fp64 in ascending rank; a point that
        coincides with a sample takes (to fp32 rounding) that sample's row.  NaN where ``nearest`` gives no neighbour.
      integer (int32 / int64 labels, one per sample): the label >= 0 most frequent among the k, on equal counts the one
        with the nearer member; -1 where there is none.  The result has the dtype of ``values``.
      any other dtype: TypeError.
    Returns (N,...), (B,N,...) or a list in the layout of ``points``.  k = 1 reproduces ``sampling.lift(values, owner)``
    wherever ``owner`` came from the same samples and distinct samples are distinct points.  Ten stream-ordered
    launches, no host synchronisation."""
    k = _k("lift_knn", k)
    p, r = _pair("lift_knn", points, samples)
    v = r.beside(values, "lift_knn", "values")
    if v.device != r.flat.device:
        raise ValueError("lift_knn: values on %s, samples on %s" % (v.device, r.flat.device))
    if v.dtype == torch.float32:
        tail = tuple(v.shape[1:])
        C = 1
        for d in tail:
            C *= int(d)
        if C < 1:
            raise ValueError("lift_knn: values of shape %s hold nothing per sample" % (tuple(v.shape),))
        idx, dist = K.knn3_query(r.flat, r, p.flat, p, k, want_dist=True)
        out = K.knn_interpolate(v.reshape(r.total, C), r, idx, dist, p).reshape((p.total,) + tail)
    elif v.dtype in (torch.int32, torch.int64):
        if v.dim() != 1:
            raise ValueError("lift_knn: integer values are labels, one per sample; got %s" % (tuple(v.shape),))
        idx = K.knn3_query(r.flat, r, p.flat, p, k)
        out = K.knn_vote(v.to(torch.int32), r, idx, p).to(v.dtype)
    else:
        raise TypeError("lift_knn: values must be float32 (interpolation) or int32 / int64 labels (vote), got %s"
                        % v.dtype)
    return p.per_point(out)
