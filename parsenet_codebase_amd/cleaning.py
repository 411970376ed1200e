"""Take the stray points out of a raw scan before anything else looks at it: statistical outlier removal on the GPU.

A scan with a handful of stray points spends its first farthest-point samples on the strays, the PCA normals next to a
stray are garbage, and the spanning-tree orientation can bridge through one.  ``outlier_statistic`` is open3d's
``remove_statistical_outlier``: a point is kept if the mean distance to its k nearest neighbours (itself included) is
positive and below mean + std_ratio * std of that statistic over its cloud.  ``remove_outliers`` applies it to the points
and to every array that runs beside them, and ``restore`` carries per-kept-point results back to the scan.

    pts, nrm, index = remove_outliers(scan, normals, search="auto")      # before everything else
    red, nrm_r, owner = reduce_cloud(pts, 10000, nrm)                    # sampling.py
    # network on red
    labels = restore(lift(labels_r, owner), index, n, -1)                # back to the n scanned points, strays -1

The definition (csrc/outlier_math.h) is exact and bit-reproducible: the fp32 neighbour distances of ``knn3_ragged`` /
``knn3_grid`` (the same bits from both), summed in fp64 in ascending order, and the two sums over a cloud taken by one
fixed tree that depends on the cloud alone.  csrc/outlier.hip runs it in six stream-ordered launches over the whole
ragged batch, without atomics, on clouds of any size.

Limits.  The statistic is global per cloud: a scan whose density varies strongly (a near and a far surface in one
cloud) loses the sparse part first.  The distances are fp32, so a point whose statistic lies within about 1e-6 relative
of the threshold may fall on the other side than with open3d's fp64 distances.  ``fitting_eval.outlier_keep_mask`` (the
fixed (20, 0.5) filter of the evaluation-mode spline segments, on fp64 distances) is a different tool and stays.
The statistic removes ISOLATED strays: a clump of thirty stray points has small neighbour distances and survives it.

A scan is rarely one shape: several parts on a table, a part and its fixture, a part and a clump of debris.
``euclidean_clusters`` labels the connected components of the graph "no further apart than a radius" (Euclidean
cluster extraction; csrc/cluster_math.h, exact, csrc/cluster.hip), ``split_clusters`` hands every object out on its own
and ``keep_largest`` keeps the object and drops the debris.  Every object then goes through the pipeline alone, at the
density the network was trained at:

    split_clusters → per object: remove_outliers → voxel_downsample → reduce_cloud → network → lift → lift → restore → restore

    for pts_c, nrm_c, index_c in split_clusters(scan, normals, radius=3 * spacing, min_size=50):
        ...                                                              # the pipeline above on pts_c
        labels = restore(labels_c, index_c, n, -1)                       # back to the n scanned points

Limits of the clusters.  A radius far above the point spacing costs the points in the ball per point and round.  Two
objects that touch (closer than the radius anywhere) are one component.  A label -1 means "dropped" (a component below
min_size), not "outlier".

Parts lie on a table, a floor or a fixture plate, every part touches that plane, and the plane links them all into one
component.  ``fit_plane`` finds the dominant plane of a cloud by RANSAC (csrc/plane_math.h, exact and
bit-reproducible; csrc/plane.hip scores every hypothesis against every point), ``remove_plane`` takes it out — or
hands it out — and ``peel_planes`` takes several, the largest first.  The tabletop recipe:

    remove_outliers → remove_plane → split_clusters → per object: voxel_downsample → reduce_cloud → network → lift → restore

(``neighbors.lift_knn(values, pts_c, reduced)`` in place of the ``lift``s: the k nearest samples instead of the one owner,
smooth along segment boundaries, and it also serves points that were never reduced — the strays, a second scan.)

    pts, nrm, index_o = remove_outliers(scan, normals, search="auto")
    pts, nrm, index_p, plane = remove_plane(pts, nrm, threshold=2 * noise, axis=(0, 0, 1), max_angle=10)
    for pts_c, nrm_c, index_c in split_clusters(pts, nrm, radius=3 * spacing, min_size=50):
        ...                                                              # the pipeline above on pts_c
        labels = restore(restore(restore(labels_c, index_c, len(pts), -1), index_p, len(index_o), -1), index_o, n, -1)

Limits of the planes.  RANSAC finds the plane with the MOST inliers, not "the floor": a wall that holds more points
wins unless ``axis`` and ``max_angle`` say which normals count.  A curved surface of low curvature (a large cylinder, a
shallow dome) can hold more points within the threshold than a small plane and win against it.  A threshold below the
sensor noise splits one plane in two: the first takes a slab of it, ``peel_planes`` finds the rest as a second plane.
The cost is hypotheses x points, whatever the cloud looks like; there is no early exit."""
import math
import numbers

import numpy as np
import torch

from . import _lib
from . import kernels as K
from .point_normals import _search
from .ragged import Clouds
from .sampling import _positive_per_cloud


def _arguments(k, std_ratio, who):
    if isinstance(k, bool) or not isinstance(k, numbers.Integral) or not K.OUTLIER_MIN_K <= k <= K.OUTLIER_MAX_K:
        raise ValueError("%s: k must be an integer %d .. %d, got %r" % (who, K.OUTLIER_MIN_K, K.OUTLIER_MAX_K, k))
    if isinstance(std_ratio, bool) or not isinstance(std_ratio, numbers.Real) or not (
            0.0 <= std_ratio and math.isfinite(std_ratio)):
        raise ValueError("%s: std_ratio must be a finite number >= 0, got %r" % (who, std_ratio))
    return int(k), float(std_ratio)


def _statistic(clouds, k, std_ratio, search, who, want_index):
    """One neighbour search and one ``K.outlier_stat`` call on checked arguments -> what ``outlier_stat`` returned."""
    search = _search(search, clouds.sizes, who)
    if clouds.total == 0:
        dist = torch.empty((0, k), dtype=torch.float32, device=clouds.flat.device)
    else:
        dist = (K.knn3_grid if search == "grid" else K.knn3_ragged)(clouds.flat, clouds, None, k, want_dist=True)[1]
    return K.outlier_stat(dist, clouds, k, std_ratio, want_index=want_index)


def outlier_statistic(points, k=20, std_ratio=2.0, search=None, return_stats=False):
    """Which points of every cloud are no statistical outliers.

    points: (N,3) or (B,N,3) fp32 on the GPU, or a list of (N_b,3) tensors (a ragged batch).
    k: neighbours per point, the point itself included, an integer 1 .. 64 (open3d's nb_neighbors).  A cloud of fewer
       than k points uses all of its points.
    std_ratio: a finite number >= 0: the threshold is mean + std_ratio * std of the statistic over the cloud.
    search: None, "grid" or "auto", the neighbour search as in ``estimate_normals`` (None: at most 10 240 points per
       cloud, a ValueError above).  The result never depends on it.
    Returns ``keep``, a bool mask in the layout of the points: (N,), (B,N) or a list of (N_b,).  With ``return_stats``
    a tuple (keep, a, stats): a, fp64 in the layout of the points, the mean distance of every point to its min(k, n)
    nearest; stats fp64, (3,), (B,3) or a list of (3,): mean, std and threshold of the cloud.  A point is kept iff
    0 < a < threshold: a point whose k nearest coincide with it is not kept (as in open3d), and a cloud of one point, or
    one whose statistic is the same everywhere, keeps nothing.  A cloud that holds a non-finite coordinate: a and stats
    NaN, nothing kept.  All results are functions of the cloud alone, whatever the batch.
    One neighbour search and one ``kernels.outlier_stat`` call (six launches), no host synchronisation."""
    who = "outlier_statistic"
    k, std_ratio = _arguments(k, std_ratio, who)
    clouds = Clouds(points, who, bad_dtype=TypeError)
    a, stats, keep, _ = _statistic(clouds, k, std_ratio, search, who, False)
    keep = clouds.per_point(keep)
    return (keep, clouds.per_point(a), clouds.per_cloud(stats)) if return_stats else keep


def remove_outliers(points, *per_point, k=20, std_ratio=2.0, search=None):
    """The one call in front of everything else: (points[index], *[a[index] for a in per_point], index).

    points, k, std_ratio, search: as in ``outlier_statistic``.  per_point: arrays with one row per point (normals,
    colours, labels) in the layout of ``points``: (N,...), (B,N,...) or lists of (N_b,...).
    ``index``, int64, holds per cloud the original row of every kept point, ascending — keep it for ``restore``.  A
    single cloud comes back as tensors; a batch or a list comes back as LISTS of tensors, one per cloud, because the
    clouds now differ in size.  A cloud may come back empty.
    Exactly one host read: the kept counts of the clouds, which size the results."""
    who = "remove_outliers"
    k, std_ratio = _arguments(k, std_ratio, who)
    clouds = Clouds(points, who, bad_dtype=TypeError)
    beside = tuple(clouds.beside(a, who, "a per-point array") for a in per_point)
    _, _, _, kept, index = _statistic(clouds, k, std_ratio, search, who, True)
    counts = _read_counts(kept)
    base = clouds.off[:-1].tolist()
    local = [index[o:o + m].long() for o, m in zip(base, counts)]                  # ascending rows of every cloud
    rows = [i + o for i, o in zip(local, base)]                                    # ... and of the flat arrays
    rows = rows[0] if len(rows) == 1 else torch.cat(rows)
    res = [a[rows] if clouds.layout == "single" else list(torch.split(a[rows], counts))
           for a in (clouds.flat,) + beside]
    return tuple(res) + (local[0] if clouds.layout == "single" else local,)


def _read_counts(kept):
    """The (S,) int32 kept counts on the host as a list: one stream-ordered download into pinned memory, one wait."""
    host, slot = _lib.pinned_like(kept.shape, kept.dtype, hold=True)
    try:
        host.copy_(kept, non_blocking=True)
        if slot is not None:
            _lib._PinnedRing.arm(slot)
            _lib.wait_event(slot["event"])
        else:
            torch.cuda.current_stream(kept.device).synchronize()
        return [int(c) for c in host.tolist()]
    finally:
        _lib._PinnedRing.release(slot)


def _cluster_arguments(points, radius, min_size, who):
    """The checks of the three cluster functions, before anything touches the GPU -> ((S,) fp32 radii on the host,
    min_size)."""
    if isinstance(points, (list, tuple)):
        S = len(points)
    else:
        S = int(points.shape[0]) if torch.is_tensor(points) and points.dim() == 3 else 1
    radii = _positive_per_cloud(radius, S, who, "radius", "number")
    if isinstance(min_size, bool) or not isinstance(min_size, numbers.Integral) or not 1 <= min_size < 2 ** 31:
        raise ValueError("%s: min_size must be an integer >= 1, got %r" % (who, min_size))
    return radii, int(min_size)


def euclidean_clusters(points, radius, min_size=1, return_info=False):
    """Which object of the scan every point belongs to: Euclidean cluster extraction (PCL's EuclideanClusterExtraction,
    open3d's cluster_dbscan with min_points = 1).

    points: (N,3) or (B,N,3) fp32 on the GPU, or a list of (N_b,3) tensors (a ragged batch).
    radius: a positive finite number, or one per cloud (host numbers: a list, an array, a CPU tensor; a GPU tensor is
       read on the host first, which is a synchronisation).  Two points belong together when a chain of points links
       them and no step of the chain is longer than the radius (fp32 squared distances against fl(radius^2); equality
       links).  A few times the point spacing is the usual choice.
    min_size: an integer >= 1; a component of fewer points is dropped.
    Returns ``label``, int32 in the layout of the points, (N,), (B,N) or a list of (N_b,): the number of every point's
    component — the kept components of a cloud are numbered 0 .. C-1 by the ascending lowest point index they hold —
    and -1 for a point of a dropped component.  With ``return_info`` a tuple (label, ncomp, count, first): ncomp int32,
    a scalar, (B,) or a list of scalars, the kept components C of every cloud; count and first, int32 in the layout of
    the points: the size and the lowest point index of component c in row c < C, -1 behind.  ncomp -1: the cloud holds a
    non-finite coordinate; -2: the square of its radius under- or overflows in fp32; both with label -1 throughout.
    All results are functions of the cloud, its radius and min_size alone (csrc/cluster_math.h), the same bits from
    run to run and for every batching.  One ``kernels.cluster_ragged`` call, no host synchronisation (with the radius
    given as host numbers)."""
    who = "euclidean_clusters"
    radii, min_size = _cluster_arguments(points, radius, min_size, who)
    clouds = Clouds(points, who, bad_dtype=TypeError)
    want = ("count", "first") if return_info else ()
    out = K.cluster_ragged(clouds.flat, clouds, _lib.h2d(radii, clouds.flat.device), min_size, want=want)
    label = clouds.per_point(out[0])
    if not return_info:
        return label
    return label, clouds.per_cloud(out[1]), clouds.per_point(out[2]), clouds.per_point(out[3])


def _components(clouds, radii, min_size, who):
    """One ``K.cluster_ragged`` call and the one host read (ncomp and the component sizes, one download) -> per cloud
    the sizes of its kept components (a list of lists) and their flat rows (a list of lists of int64 tensors, the rows
    of every component ascending).  Raises ValueError for a cloud with status -2; one with -1 has no component."""
    dev = clouds.flat.device
    label, ncomp, count = K.cluster_ragged(clouds.flat, clouds, _lib.h2d(radii, dev), min_size, want=("count",))
    host = _read_counts(torch.cat([ncomp, count]))
    S, base = clouds.S, clouds.off[:-1].tolist()
    for c, v in enumerate(host[:S]):
        if v == -2:
            raise ValueError("%s: cloud %d: the square of radius = %r is no positive finite fp32 number"
                             % (who, c, float(radii[c])))
    found = [max(v, 0) for v in host[:S]]
    sizes = [host[S + o:S + o + v] for o, v in zip(base, found)]
    flat_sizes = [m for part in sizes for m in part]
    if not flat_sizes:
        return sizes, [[] for _ in range(S)]
    # a stable sort by (cloud, component) keeps the rows of every component ascending; dropped points go last
    before = np.cumsum([0] + found[:-1])
    shift = torch.repeat_interleave(_lib.h2d(before.astype(np.int64), dev),
                                    _lib.h2d(np.asarray(clouds.sizes, dtype=np.int64), dev), output_size=clouds.total)
    key = torch.where(label >= 0, label.long() + shift, len(flat_sizes))
    rows = torch.sort(key, stable=True).indices[:sum(flat_sizes)]
    pieces = iter(torch.split(rows, flat_sizes))
    return sizes, [[next(pieces) for _ in part] for part in sizes]


def split_clusters(points, *per_point, radius, min_size=1, order="index"):
    """Take a scan apart into its objects, in front of everything else: for every kept component
    (points[index], *[a[index] for a in per_point], index).

    points, radius, min_size: as in ``euclidean_clusters``.  per_point: arrays with one row per point (normals, colours,
    labels) in the layout of ``points``.  order: "index" — the components in the order of their lowest point, as they
    are numbered — or "size" — the largest first, ties by the lowest point.
    One cloud gives a list over its components; a batch or a list of clouds gives a list of such lists.  ``index``,
    int64, holds the original rows of the component, ascending — keep it for ``restore``.  Points of components below
    min_size are in no component.  A cloud that holds a non-finite coordinate gives no component; a radius whose square
    under- or overflows in fp32 raises ValueError, naming the cloud.
    Exactly one host read: the number of components and their sizes, which size the results."""
    who = "split_clusters"
    if order not in ("index", "size"):
        raise ValueError('%s: order must be "index" or "size", got %r' % (who, order))
    radii, min_size = _cluster_arguments(points, radius, min_size, who)
    clouds = Clouds(points, who, bad_dtype=TypeError)
    beside = tuple(clouds.beside(a, who, "a per-point array") for a in per_point)
    sizes, rows = _components(clouds, radii, min_size, who)
    out = []
    for o, part, m in zip(clouds.off[:-1].tolist(), rows, sizes):
        ranks = range(len(part)) if order == "index" else sorted(range(len(part)), key=lambda c: (-m[c], c))
        out.append([tuple(a[part[c]] for a in (clouds.flat,) + beside) + (part[c] - o,) for c in ranks])
    return out[0] if clouds.layout == "single" else out


def keep_largest(points, *per_point, radius):
    """The object of the scan, without the debris around it: (points[index], *[a[index] for a in per_point], index) of
    the largest connected component of every cloud, ties by the lowest point — the shape of ``remove_outliers``, whose
    statistic a clump of stray points survives.  points, radius, per_point: as in ``split_clusters``.  A single cloud
    comes back as tensors, a batch or a list as LISTS of tensors, one per cloud; ``index``, int64, ascending, is ready
    for ``restore``.  An empty cloud, or one that holds a non-finite coordinate, comes back empty; a radius whose
    square under- or overflows in fp32 (1e-30) raises ValueError, naming the cloud, as in ``split_clusters``.  Exactly
    one host read."""
    who = "keep_largest"
    radii, _ = _cluster_arguments(points, radius, 1, who)
    clouds = Clouds(points, who, bad_dtype=TypeError)
    beside = tuple(clouds.beside(a, who, "a per-point array") for a in per_point)
    sizes, rows = _components(clouds, radii, 1, who)
    none = torch.empty(0, dtype=torch.int64, device=clouds.flat.device)
    picked = [part[max(range(len(part)), key=lambda c: (m[c], -c))] if part else none for part, m in zip(rows, sizes)]
    res = [[a[p] for p in picked] for a in (clouds.flat,) + beside]
    res.append([p - o for p, o in zip(picked, clouds.off[:-1].tolist())])
    return tuple(part[0] if clouds.layout == "single" else part for part in res)


def _plane_arguments(points, threshold, who):
    """The threshold check of the plane functions, before anything touches the GPU -> (S,) fp32 on the host."""
    if isinstance(points, (list, tuple)):
        S = len(points)
    else:
        S = int(points.shape[0]) if torch.is_tensor(points) and points.dim() == 3 else 1
    return _positive_per_cloud(threshold, S, who, "threshold", "number")


def _fit(clouds, thresholds, hypotheses, seed, refine, axis, max_angle, want):
    return K.plane_ragged(clouds.flat, clouds, _lib.h2d(thresholds, clouds.flat.device), hypotheses, seed, refine, axis,
                          max_angle, want=want)


def fit_plane(points, threshold, hypotheses=512, seed=0, refine=1, axis=None, max_angle=None, return_info=False):
    """The dominant plane of every cloud — the table, the floor, the fixture plate — by RANSAC (PCL's
    SACSegmentation with SACMODEL_PLANE / SACMODEL_PERPENDICULAR_PLANE, open3d's segment_plane).

    points: (N,3) or (B,N,3) fp32 on the GPU, or a list of (N_b,3) tensors (a ragged batch).
    threshold: a positive finite number, or one per cloud (host numbers, as the radius of ``euclidean_clusters``): a
       point belongs to a plane when it is no further from it than this.  The sensor noise sets it.
    hypotheses: 1 .. 4096 planes through three points of the cloud are tried; seed: an integer, which fixes the draws.
    refine: 0 .. 4 rounds of a least-squares plane through the inliers; a round is taken only if it loses no inlier.
    axis, max_angle: three numbers and degrees 0 .. 90, together or not at all: only planes whose normal is within
       max_angle of +-axis are considered (axis=(0,0,1), max_angle=10: the floor, not the wall).
    Returns (plane, inlier): plane fp64, (4,), (B,4) or a list of (4,): nx, ny, nz, d with n . p + d = 0, |n| = 1 and
    the component of n of largest magnitude positive; inlier, a bool mask in the layout of the points.  With
    ``return_info`` a tuple (plane, inlier, count, best, dist): count int32, a scalar, (B,) or a list: the inliers, -1
    for a cloud that holds a non-finite coordinate; best int32 likewise: the winning hypothesis, -1 where none is valid
    (fewer than three points, a collinear cloud, an axis that excludes every sample: plane zeros, no inlier, dist NaN);
    dist fp32 in the layout of the points: the signed distance of every point to the plane.
    All results are functions of the cloud and the arguments alone (csrc/plane_math.h), the same bits from run to run
    and for every batching.  One ``kernels.plane_ragged`` call, no host synchronisation."""
    who = "fit_plane"
    thresholds = _plane_arguments(points, threshold, who)
    clouds = Clouds(points, who, bad_dtype=TypeError)
    out = _fit(clouds, thresholds, hypotheses, seed, refine, axis, max_angle, ("dist",) if return_info else ())
    plane, inlier = clouds.per_cloud(out[0]), clouds.per_point(out[3])
    if not return_info:
        return plane, inlier
    return plane, inlier, clouds.per_cloud(out[1]), clouds.per_cloud(out[2]), clouds.per_point(out[4])


def remove_plane(points, *per_point, threshold, keep="rest", hypotheses=512, seed=0, refine=1, axis=None,
                 max_angle=None):
    """Take the dominant plane out of a scan: (points[index], *[a[index] for a in per_point], index, plane).

    points, threshold, hypotheses, seed, refine, axis, max_angle: as in ``fit_plane``.  per_point: arrays with one row
    per point in the layout of ``points``.  keep: "rest" — everything but the inliers of the plane — or "plane" — the
    inliers.  ``index``, int64, holds per cloud the original row of every point handed out, ascending — keep it for
    ``restore``; ``plane`` is the plane of ``fit_plane``.  A single cloud comes back as tensors; a batch or a list comes
    back as LISTS of tensors, one per cloud.  A cloud that holds a non-finite coordinate, or in which no hypothesis is
    valid, has no plane: it keeps all its points under "rest" and none under "plane".
    Exactly one host read: the inlier counts of the clouds, which size the results."""
    who = "remove_plane"
    if keep not in ("rest", "plane"):
        raise ValueError('%s: keep must be "rest" or "plane", got %r' % (who, keep))
    thresholds = _plane_arguments(points, threshold, who)
    clouds = Clouds(points, who, bad_dtype=TypeError)
    beside = tuple(clouds.beside(a, who, "a per-point array") for a in per_point)
    plane, count, _, inlier = _fit(clouds, thresholds, hypotheses, seed, refine, axis, max_angle, ())
    host = _read_counts(count)
    for c, v in enumerate(host):
        if v == -2:
            raise ValueError("%s: cloud %d: threshold = %r is no positive finite fp32 number"
                             % (who, c, float(thresholds[c])))
    found = [max(v, 0) for v in host]
    counts = found if keep == "plane" else [n - m for n, m in zip(clouds.sizes, found)]
    # a stable sort by "handed out first" keeps the rows ascending, cloud after cloud
    last = (inlier if keep == "rest" else ~inlier).to(torch.uint8)
    rows = torch.sort(last, stable=True).indices[:sum(counts)]
    base = clouds.off[:-1].tolist()
    res = [a[rows] if clouds.layout == "single" else list(torch.split(a[rows], counts))
           for a in (clouds.flat,) + beside]
    local = [r - o for r, o in zip(torch.split(rows, counts), base)]
    return tuple(res) + (local[0] if clouds.layout == "single" else local, clouds.per_cloud(plane))


def peel_planes(points, *per_point, threshold, max_planes, min_inliers, hypotheses=512, seed=0, refine=1, axis=None,
                max_angle=None):
    """The planes of ONE cloud, the largest first: ``remove_plane`` on what is left, up to ``max_planes`` times.

    points (N,3) and per_point (N,...): one cloud.  It stops at the first plane with fewer than ``min_inliers`` inliers
    (an integer >= 1), which is not handed out; round p uses seed + p.  The other arguments as in ``fit_plane``.
    Returns (planes, rest): planes, a list of (points_p, *per_point_p, index_p, plane_p), and rest, (points_r,
    *per_point_r, index_r): what no plane took.  Every index, int64 ascending, refers to the ORIGINAL rows; the indices
    are disjoint and together hold every row.
    One host read per plane tried (the inlier count, inside ``remove_plane``)."""
    who = "peel_planes"
    if not torch.is_tensor(points) or points.dim() != 2:
        raise ValueError("%s: one cloud (N,3)" % who)
    for name, v in (("max_planes", max_planes), ("min_inliers", min_inliers)):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not 1 <= v < 2 ** 31:
            raise ValueError("%s: %s must be an integer >= 1, got %r" % (who, name, v))
    if isinstance(seed, bool) or not isinstance(seed, numbers.Integral):
        raise ValueError("%s: seed must be an integer, got %r" % (who, seed))
    clouds = Clouds(points, who, bad_dtype=TypeError)
    left = (clouds.flat,) + tuple(clouds.beside(a, who, "a per-point array") for a in per_point)
    origin = torch.arange(clouds.total, dtype=torch.int64, device=clouds.flat.device)
    planes = []
    for p in range(int(max_planes)):
        out = remove_plane(*left, origin, threshold=threshold, keep="plane", hypotheses=hypotheses,
                           seed=(seed + p) & (2 ** 64 - 1), refine=refine, axis=axis, max_angle=max_angle)
        local = out[-2]
        if local.shape[0] < min_inliers:
            break
        planes.append(tuple(out[:-3]) + (out[-3], out[-1]))
        rest = torch.ones(left[0].shape[0], dtype=torch.bool, device=local.device)
        rest[local] = False
        left, origin = tuple(a[rest] for a in left), origin[rest]
    return planes, left + (origin,)


def restore(values, index, n, fill):
    """Per-kept-point values back to the n points of the scan: out[index] = values, ``fill`` everywhere else.

    values: (kept,...) — labels, ``lift``ed results, anything with one row per kept point —, index: (kept,) int64 as
    ``remove_outliers`` returned it, n: the points of the scan; or lists of as many tensors, n an int or one int per
    cloud.  Returns (n,...) in the dtype of ``values``, or a list.  Raises ValueError for an index outside 0 .. n - 1
    (one host read per cloud)."""
    if isinstance(index, (list, tuple)):
        if not isinstance(values, (list, tuple)) or len(values) != len(index):
            raise ValueError("restore: a list of indices takes a list of as many value tensors")
        ns = list(n) if isinstance(n, (list, tuple)) else [n] * len(index)
        if len(ns) != len(index):
            raise ValueError("restore: n holds one size per cloud (%d)" % len(index))
        return [restore(v, i, m, fill) for v, i, m in zip(values, index, ns)]
    if not torch.is_tensor(values) or not torch.is_tensor(index):
        raise TypeError("restore: values and index must be tensors or lists of tensors")
    if index.dtype not in (torch.int64, torch.int32):
        raise TypeError("restore: index must be an integer tensor, got %s" % index.dtype)
    if isinstance(n, bool) or not isinstance(n, numbers.Integral) or n < 0:
        raise ValueError("restore: n must be an integer >= 0, got %r" % (n,))
    if index.dim() != 1 or values.dim() < 1 or values.shape[0] != index.shape[0]:
        raise ValueError("restore: index (kept,) with values (kept,...); got %s and %s"
                         % (tuple(index.shape), tuple(values.shape)))
    if index.numel() and (int(index.min()) < 0 or int(index.max()) >= n):
        raise ValueError("restore: index holds a row outside the %d points" % n)
    out = torch.full((int(n),) + tuple(values.shape[1:]), fill, dtype=values.dtype, device=values.device)
    out[index.long()] = values
    return out
