"""Reduce a scan of any size to the network's size and carry the results back: farthest-point sampling on the GPU.

The segmentation network, the mean-shift stage and the fitting stage are built around some 10 000 points per shape; a
raw scan holds a hundred times as many.  A random choice (``trainer._subsample``) reproduces the scan's uneven density
and drops thin parts.  ``farthest_point_sample`` picks m points that cover the cloud — every next sample is the point
farthest from the samples so far — and, while it runs, knows for every scanned point which sample is nearest: that
"owner" is the lift of per-sample results (labels, primitive ids, membership rows) back to full resolution.

    reduced, normals_r, owner = reduce_cloud(scan, 10000, normals)      # before the network
    labels_full = lift(labels_of_reduced, owner)                        # after it

The definition (csrc/fps_math.h) is exact and bit-reproducible: squared distances
((x_i-x_j)^2 + (y_i-y_j)^2) + (z_i-z_j)^2 rounded once per operation in fp32, strict updates, the lowest index on equal
distances.  csrc/fps.hip runs it from global memory over many workgroups, so no cloud size is a limit.

Limits.  The sampling is sequential in m: m + 2 stream-ordered launches.  It picks outliers first: a scan with stray
points goes through ``cleaning.remove_outliers`` before it.  ``owner`` is the nearest SAMPLE, not a surface projection:
lifting labels across a thin wall follows Euclidean distance.  ``neighbors.lift_knn(values, points, reduced, k=3)`` ends
the pipeline instead of ``lift`` where segment boundaries should be smooth (the k nearest samples, weighted or voting)
and for points that were never reduced and so have no ``owner``.

A dense, unevenly sampled scan goes through ``voxel_downsample`` first: one point per occupied cell of a cubic grid
(csrc/voxel_math.h, csrc/voxel.hip: exact centroids from 64-bit integer sums, seven launches whatever the size), which
equalises the density and leaves the sequential sampling a tenth of the points.  The two owners compose:

    vox, nrm_v, own_v = voxel_downsample(pts, h, nrm, position="point")
    red, nrm_r, own_f = reduce_cloud(vox, 10000, nrm_v)
    labels = lift(lift(labels_r, own_f), own_v)"""
import numbers

import numpy as np
import torch

from . import _lib
from . import kernels as K
from .ragged import Clouds


def _starts(start, S, device, who):
    """None, an int or one int per cloud -> None or (S,) int32 on the device."""
    if start is None:
        return None
    if isinstance(start, numbers.Integral) and not isinstance(start, bool):
        start = [int(start)] * S
    elif isinstance(start, (list, tuple, np.ndarray)) or torch.is_tensor(start):
        start = start.tolist() if isinstance(start, np.ndarray) or torch.is_tensor(start) else list(start)
        if not isinstance(start, list) or len(start) != S:
            raise ValueError("%s: start holds one index per cloud (%d)" % (who, S))
        if not all(isinstance(s, numbers.Integral) and not isinstance(s, bool) for s in start):
            raise ValueError("%s: start must be None, an int or one int per cloud, got %r" % (who, start))
    else:
        raise ValueError("%s: start must be None, an int or one int per cloud, got %r" % (who, start))
    return _lib.h2d(np.clip(np.asarray(start, dtype=np.int64), -2 ** 31, 2 ** 31 - 1).astype(np.int32), device)


def _samples(points, m, start, who, want_owner, want_radius, full=False):
    """The clouds as a ``Clouds`` (a non-fp32 dtype is a TypeError here) and the tuple ``K.fps_ragged`` returns."""
    if isinstance(m, bool) or not isinstance(m, numbers.Integral) or m < 1:
        raise ValueError("%s: m must be an integer >= 1, got %r" % (who, m))
    clouds = Clouds(points, who, bad_dtype=TypeError)
    if clouds.S == 0:
        raise ValueError("%s: an empty batch of clouds" % who)
    if full and min(clouds.sizes) < m:
        raise ValueError("%s: a cloud of %d points cannot give m = %d samples" % (who, min(clouds.sizes), m))
    start = _starts(start, clouds.S, clouds.flat.device, who)
    out = K.fps_ragged(clouds.flat, clouds, None, int(m), start=start, want_owner=want_owner, want_radius=want_radius)
    return clouds, (out if isinstance(out, tuple) else (out,))


def farthest_point_sample(points, m, start=None, return_owner=False, return_radius=False):
    """Farthest-point sampling of every cloud.

    points: (N,3) or (B,N,3) fp32 on the GPU, or a list of (N_b,3) tensors (a ragged batch).
    m: samples per cloud, >= 1.  A cloud of n < m points gives its n points and -1 in the other entries.
    start: the first sample — None (point 0), an int, or one int per cloud; clamped into the cloud.
    Returns ``sample``, int64 indices into the cloud in selection order: (m,), (B,m) or a list of (m,), so that
    ``points[sample]`` works on a single cloud.  With ``return_owner`` also ``owner`` (int64, per point: the rank in
    ``sample`` of the nearest sample, ties to the earliest) and ``dist`` (fp32, the squared distance to it), in the
    layout of the points: (N,), (B,N) or a list.  With ``return_radius`` also ``radius`` last, in the layout of
    ``sample``: the squared distance of every sample to the earlier ones when it was chosen (+inf first, then
    non-increasing; the last one bounds every ``dist``), NaN where ``sample`` is -1.
    A cloud that holds a non-finite coordinate gets -1 and NaN throughout.  All results are functions of the input
    alone.  m + 2 stream-ordered launches, no host synchronisation."""
    who = "farthest_point_sample"
    clouds, out = _samples(points, m, start, who, return_owner, return_radius)
    res = [clouds.per_cloud(out[0].long())]
    if return_owner:
        res += [clouds.per_point(out[1].long()), clouds.per_point(out[2])]
    if return_radius:
        res.append(clouds.per_cloud(out[-1]))
    return tuple(res) if len(res) > 1 else res[0]


def reduce_cloud(points, m, *per_point, start=None):
    """The one call in front of the network: (points[sample], *[a[sample] for a in per_point], owner).

    points, m, start: as in ``farthest_point_sample``.  per_point: arrays with one row per point (normals, colours,
    labels) in the layout of ``points``: (N,...), (B,N,...) or lists of (N_b,...).  The reduced arrays come back as
    (m,...), (B,m,...) or lists of (m,...); ``owner`` as in ``farthest_point_sample`` — keep it for ``lift``.
    Raises ValueError if a cloud has fewer than m points (a -1 index would gather the wrong row silently)."""
    who = "reduce_cloud"
    clouds, out = _samples(points, m, start, who, True, False, full=True)
    rows = (out[0] + clouds.device_offsets()[:-1, None]).long().reshape(-1)            # rows of the flat arrays
    res = []
    for a in (clouds.flat,) + tuple(clouds.beside(a, who, "a per-point array") for a in per_point):
        res.append(clouds.per_cloud(a[rows].reshape((clouds.S, int(m)) + tuple(a.shape[1:]))))
    return tuple(res) + (clouds.per_point(out[1].long()),)


def _positive(v):
    """Is v a number (no bool) that is positive and finite as fp32?"""
    if isinstance(v, bool) or not isinstance(v, numbers.Real):
        return False
    try:
        with np.errstate(over="ignore"):
            f = np.float32(v)
    except OverflowError:
        return False
    return bool(f > 0 and np.isfinite(f))


def _positive_per_cloud(value, S, who, name, noun):
    """A positive finite number or one per cloud -> (S,) fp32 on the host; ``name`` and ``noun`` word the errors
    ("voxel holds one size per cloud").  A tensor is read on the host (a GPU tensor: one synchronisation)."""
    if isinstance(value, (list, tuple, np.ndarray)) or torch.is_tensor(value):
        each = value.tolist() if isinstance(value, np.ndarray) or torch.is_tensor(value) else list(value)
        if not isinstance(each, list):
            each = [each] * S                                                     # (a 0-d array or tensor)
        elif len(each) != S:
            raise ValueError("%s: %s holds one %s per cloud (%d), got %d" % (who, name, noun, S, len(each)))
    else:
        each = [value] * S
    if not all(_positive(v) for v in each):
        raise ValueError("%s: %s must be a positive finite number or one per cloud, got %r" % (who, name, value))
    return np.asarray(each, dtype=np.float32)


def _voxel_sizes(voxel, S, who):
    """A positive finite number or one per cloud -> (S,) fp32 on the host."""
    return _positive_per_cloud(voxel, S, who, "voxel", "size")


def _voxel_origins(origin, S, who):
    """None, 3 numbers or 3 per cloud -> None or (S,3) fp32 on the host."""
    if origin is None:
        return None
    try:
        if torch.is_tensor(origin):
            origin = origin.detach().cpu().numpy()
        if isinstance(origin, (str, bytes)) or any(isinstance(v, bool) for v in np.asarray(origin, object).ravel()):
            raise TypeError
        with np.errstate(over="ignore"):
            o = np.asarray(origin, dtype=np.float64).astype(np.float32)
    except (TypeError, ValueError):
        o = None
    if o is not None and o.shape == (3,):
        o = np.tile(o, (S, 1))
    if o is None or o.shape != (S, 3) or not np.isfinite(o).all():
        raise ValueError("%s: origin must be None, 3 finite numbers or 3 per cloud (%d), got %r" % (who, S, origin))
    return np.ascontiguousarray(o)


def voxel_downsample(points, voxel, *per_point, origin=None, position="centroid", return_info=False):
    """The first step on a dense scan: one point per occupied cell of a cubic grid, and for every scanned point the
    voxel that holds it.  (reduced, *[a[rep] for a in per_point], owner).

    points: (N,3) or (B,N,3) fp32 on the GPU, or a list of (N_b,3) tensors (a ragged batch).
    voxel: the edge of the cells, a positive finite number, or one per cloud.
    origin: a corner of the grid — None (the per-axis minimum of every cloud), 3 numbers, or 3 per cloud.  The cell of
       a point is floor((x - origin) / voxel) per axis, in fp64; a point on a face belongs to the upper cell.
    position: "centroid" — ``reduced`` holds the exact mean of every voxel's points, which averages sensor noise away
       — or "point" — ``reduced`` is ``points[rep]``, rep the point of the voxel nearest to its centroid: actual scan
       points, which lie on the surface.
    per_point: arrays with one row per point (normals, colours, labels) of any dtype, in the layout of ``points``:
       (N,...), (B,N,...) or lists of (N_b,...).  They are GATHERED at the representative, exact rows — right for
       labels, and right for normals at a crease.  Averaged attributes per voxel are out of scope.
    Voxels are numbered by the ascending lowest point index they hold.  ``owner``, int64 in the layout of the points,
    (N,), (B,N) or a list, is the number of every point's voxel — keep it for ``lift``.  With ``return_info`` also
    ``count`` and ``rep`` (int64, per voxel: its points, and the index of its representative in the cloud) last.
    A single cloud comes back as tensors; a batch or a list comes back as LISTS of tensors, one per cloud, because the
    voxel counts differ (as in ``cleaning.remove_outliers``).  A cloud that holds a non-finite coordinate gives zero
    voxels and owner -1, which ``lift`` refuses.  Raises ValueError ("voxel too small", naming the cloud) where a cell
    index leaves -2^20 .. 2^20 - 1.  All results are functions of the cloud, the voxel and the origin alone
    (csrc/voxel_math.h).  Seven stream-ordered launches and exactly one host read: the voxel counts, which size the
    results."""
    who = "voxel_downsample"
    if position not in ("centroid", "point"):
        raise ValueError('%s: position must be "centroid" or "point", got %r' % (who, position))
    if isinstance(points, (list, tuple)):
        S = len(points)
    else:
        S = int(points.shape[0]) if torch.is_tensor(points) and points.dim() == 3 else 1
    sizes, origins = _voxel_sizes(voxel, S, who), _voxel_origins(origin, S, who)
    clouds = Clouds(points, who, bad_dtype=TypeError)
    beside = tuple(clouds.beside(a, who, "a per-point array") for a in per_point)
    dev = clouds.flat.device
    want = (("centroid",) if position == "centroid" else ()) + (("count",) if return_info else ()) + ("rep",)
    out = K.voxel_ragged(clouds.flat, clouds, _lib.h2d(sizes, dev), None if origins is None else _lib.h2d(origins, dev),
                         want=want)
    found = dict(zip(("owner", "nvox") + want, out))
    from .cleaning import _read_counts
    counts = _read_counts(found["nvox"])
    for c, v in enumerate(counts):
        if v == -2:
            raise ValueError("%s: cloud %d: voxel too small for the extent of the cloud (a cell index outside "
                             "-2^20 .. 2^20 - 1), voxel = %r" % (who, c, float(sizes[c])))
    counts = [max(v, 0) for v in counts]
    base = clouds.off[:-1].tolist()
    head = [torch.arange(o, o + v, device=dev) for o, v in zip(base, counts)]       # the voxel rows of every cloud
    first = [torch.full((v,), o, dtype=torch.int64, device=dev) for o, v in zip(base, counts)]
    head, first = (part[0] if len(part) == 1 else torch.cat(part) for part in (head, first))
    rep = found["rep"][head].long()                                                 # LOCAL to the cloud
    rows = rep + first                                                              # ... and of the flat arrays
    reduced = found["centroid"][head] if position == "centroid" else clouds.flat[rows]
    res = [reduced] + [a[rows] for a in beside]
    info = [found["count"][head].long(), rep] if return_info else []
    single = clouds.layout == "single"
    res, info = ([a if single else list(torch.split(a, counts)) for a in part] for part in (res, info))
    return tuple(res) + (clouds.per_point(found["owner"].long()),) + tuple(info)


def lift(values, owner):
    """Per-sample values to per-point values: ``values[owner]`` per cloud, over any trailing shape.

    values: (m,...), (B,m,...) or a list of (m_b,...) tensors — labels, primitive ids, membership rows of the reduced
    cloud; owner: what ``farthest_point_sample`` / ``reduce_cloud`` returned, (N,), (B,N) or a list of (N_b,).
    Returns (N,...), (B,N,...) or a list.  Raises ValueError where owner holds -1 (a cloud with a non-finite
    coordinate) or a rank past the values."""
    if isinstance(owner, (list, tuple)):
        if not isinstance(values, (list, tuple)) or len(values) != len(owner):
            raise ValueError("lift: a list of owners takes a list of as many value tensors")
        return [lift(v, o) for v, o in zip(values, owner)]
    if not torch.is_tensor(owner) or not torch.is_tensor(values):
        raise TypeError("lift: values and owner must be tensors or lists of tensors")
    if owner.dtype not in (torch.int64, torch.int32):
        raise TypeError("lift: owner must be an integer tensor, got %s" % owner.dtype)
    if owner.dim() not in (1, 2) or values.dim() < owner.dim() or (owner.dim() == 2
                                                                    and values.shape[0] != owner.shape[0]):
        raise ValueError("lift: owner (N,) with values (m,...), or owner (B,N) with values (B,m,...); got %s and %s"
                         % (tuple(owner.shape), tuple(values.shape)))
    m = values.shape[owner.dim() - 1]
    if owner.numel() and (int(owner.min()) < 0 or int(owner.max()) >= m):
        raise ValueError("lift: owner holds -1 or a rank past the %d values (a cloud without samples?)" % m)
    owner = owner.long()
    if owner.dim() == 1:
        return values[owner]
    B, N = owner.shape
    rows = (owner + torch.arange(B, device=owner.device)[:, None] * m).reshape(-1)
    return values.reshape((B * m,) + tuple(values.shape[2:]))[rows].reshape((B, N) + tuple(values.shape[2:]))
