"""Rigid registration of two scans on the GPU: bring a second scan of a part into the frame of the first.

``register`` is iterative closest point (ICP) on the exact cross-cloud search of ``neighbors.nearest``
(csrc/register.hip, definition csrc/register_math.h): the target's grid is built once, and every iteration moves the
source, pairs every moved point with its nearest target point, sums the accepted pairs in fp64 over one fixed tree and
solves for the step — Horn's quaternion (``method="point"``) or the linearised point-to-plane step
(``method="plane"``, which slides along flat regions and needs fewer iterations) — with the stopping rule decided per
cloud on the device.  ``apply_transform`` moves points (and rotates normals) by the result, ``register_pyramid`` runs
coarse to fine on voxel-downsampled copies.

    normals = estimate_normals(target)                                        # orientation does not matter
    T = register(source, target, max_dist=0.05, method="plane", target_normals=normals)
    merged = torch.cat([apply_transform(source, T), target])
    merged, owner = voxel_downsample(merged, voxel)                           # one cloud, one density

Every function takes (N,3), (B,N,3) or a list of (N_b,3) fp32 clouds on the GPU; source and target may differ in layout
and sizes but must hold the same number of clouds: cloud s of the source is registered onto cloud s of the target.  All
results are functions of the inputs alone, the same bits from run to run and for every batching.

Limits.  ICP is a LOCAL minimiser: it needs an ``init``, a small motion (a few degrees and a fraction of the part's
size), or the pyramid; from further away it converges — with status "converged" — to a wrong pose.  A symmetric shape
has many minima.  The pairs follow the Euclidean distance.  A source point far outside the target's box costs what the
``neighbors`` module says of such queries (many rings: slow, never wrong).  Plane mode needs target normals; their
orientation does not matter."""
import numbers

import torch

from . import _lib, kernels as K
from .neighbors import _pair

STATUS_NAMES = {0: "converged", 1: "max_iter", 2: "too_few", 3: "degenerate", 4: "non_finite"}
_METHODS = {"point": K.REGISTER_POINT, "plane": K.REGISTER_PLANE}


def _init(who, init, S, device):
    """None, or (S,4,4) float64 on ``device`` from a (4,4) / (S,4,4) float64 tensor.  A host tensor goes up through
    the pinned staging ring (``_lib.h2d``), one stream-ordered copy that does not make the host wait."""
    if init is None:
        return None
    if not torch.is_tensor(init) or init.dtype != torch.float64:
        raise TypeError("%s: init must be a float64 tensor of shape (4,4) or (B,4,4)" % who)
    if tuple(init.shape) == (4, 4):
        init = init.expand(S, 4, 4)
    if tuple(init.shape) != (S, 4, 4):
        raise ValueError("%s: init must be (4,4) or (%d,4,4), got %s" % (who, S, tuple(init.shape)))
    if not init.is_cuda:
        return _lib.h2d(init.contiguous().numpy(), device)
    return init.to(device)


def register(source, target, max_dist, init=None, method="point", target_normals=None, max_iter=50, tol_rot=1e-6,
             tol_trans=1e-6, return_info=False):
    """The rigid transform that moves ``source`` onto ``target``: (4,4) float64 for one cloud, (B,4,4) for a batch or a
    list, on the GPU.

    max_dist: pairs further apart are ignored (fp32, >= 0; ``float("inf")`` takes every pair) — set it to a few times the
       expected misalignment so that the parts of the source the target does not cover drop out.
    init: a (4,4) or (B,4,4) float64 start, None for the identity; on the GPU, or on the host (then uploaded through
       pinned memory in one stream-ordered copy).
    method: "point", or "plane" with ``target_normals`` in the layout of the target (from ``estimate_normals``).
    max_iter 1 .. 256; the iteration stops per cloud once a step rotates by at most tol_rot (radians) and moves the
       centroid of the paired points by at most tol_trans.
    With ``return_info`` also a dict: iterations, status (int32 per cloud, see STATUS_NAMES), count and rmse (the accepted
    pairs of the final transform and their root mean square distance, float64; NaN without pairs) as (B,) tensors —
    0-dim for a single cloud —, and idx (int64, -1: no pair found) and dist (fp32) per source point in the layout of the
    source.  Check status: a cloud that stopped as "too_few", "degenerate" or "non_finite" returns the transform it
    had.  12 + 9 max_iter stream-ordered launches whatever the clouds do — a stopped cloud's workgroups exit at once —
    and no host synchronisation."""
    who = "register"
    if method not in _METHODS:
        raise ValueError('%s: method must be "point" or "plane", got %r' % (who, method))
    if method == "plane" and target_normals is None:
        raise ValueError('%s: method "plane" needs target_normals' % who)
    if method == "point" and target_normals is not None:
        raise ValueError('%s: target_normals are read by method "plane" only' % who)
    max_dist = K._nonneg(who, "max_dist", max_dist, allow_inf=True)
    tol_rot, tol_trans = K._nonneg(who, "tol_rot", tol_rot), K._nonneg(who, "tol_trans", tol_trans)
    if isinstance(max_iter, bool) or not isinstance(max_iter, numbers.Integral) or not 1 <= max_iter <= K.REGISTER_MAX_ITER:
        raise ValueError("%s: max_iter must be an integer 1 .. %d, got %r" % (who, K.REGISTER_MAX_ITER, max_iter))
    if init is not None and (not torch.is_tensor(init) or init.dtype != torch.float64 or init.dim() not in (2, 3)
                             or tuple(init.shape[-2:]) != (4, 4)):
        raise ValueError("%s: init must be a float64 tensor of shape (4,4) or (B,4,4)" % who)
    s, t = _pair(who, source, target)
    normals = None if target_normals is None else t.beside(target_normals, who, "target_normals")
    out = K.register_ragged(s.flat, s, t.flat, t, max_dist, _METHODS[method], normals, _init(who, init, s.S, s.flat.device),
                            max_iter, tol_rot, tol_trans, want_pairs=return_info)
    single = s.layout == "single"
    T = out[0][0] if single else out[0]
    if not return_info:
        return T
    info = dict(zip(("iterations", "status", "count", "rmse"), (v[0] if single else v for v in out[1:5])))
    info["idx"], info["dist"] = s.per_point(out[5].long()), s.per_point(out[6])
    return T, info


def apply_transform(points, transform, *normals):
    """``points`` moved by ``transform`` — (4,4), or (B,4,4) with one per cloud, float64 — and, after them, every array
    of ``normals`` (fp32, in the layout of the points) rotated only.  The points go through the move step of ``register``
    itself (pn_rigid_apply_f32: fp64 arithmetic, rounded to fp32 once, the rotation re-derived from the unit quaternion of
    the 3 x 3 block, so a block that is no rotation is replaced by one).  Returns the moved points, or
    (points, *normals), in the layout they came in."""
    from .ragged import Clouds
    who = "apply_transform"
    p = Clouds(points, who, bad_dtype=TypeError)
    if not torch.is_tensor(transform) or transform.dtype != torch.float64:
        raise TypeError("%s: transform must be a float64 tensor of shape (4,4) or (B,4,4)" % who)
    T = _init(who, transform, p.S, p.flat.device)
    moved = K.rigid_apply(p.flat, p, T.contiguous())
    if not normals:
        return p.per_point(moved)
    zero = T.clone()
    zero[:, :3, 3] = 0.0
    out = [p.per_point(moved)]
    for n in normals:
        out.append(p.per_point(K.rigid_apply(p.beside(n, who, "normals").contiguous(), p, zero)))
    return tuple(out)


def register_pyramid(source, target, voxels, max_dist_factor=3.0, init=None, **kw):
    """Coarse to fine: for every voxel size of ``voxels`` (give them descending) both clouds are reduced by
    ``sampling.voxel_downsample`` to one centroid per cell and registered with ``max_dist = max_dist_factor * voxel``,
    starting from the previous level's transform (the first from ``init``).  A coarse level accepts distant pairs on few
    points and tolerates a start from which ``register`` with the last level's ``max_dist`` finds too few true pairs;
    the last level decides the accuracy — the centroids of two scans are not the same points, so end with a voxel near
    the scans' resolution.  Keep the coarsest voxel below the size of the detail that makes the part asymmetric: a
    level that no longer sees it slides along the symmetry, and the finer levels' ``max_dist`` may not bring it back.
    ``kw`` goes to ``register`` (method="plane" takes target_normals in the layout of the target: they are gathered at
    every voxel's representative point, and the target is then reduced to those points, not to centroids).  Returns what
    ``register`` returns for the last level; with return_info its idx and dist refer to the LAST level's reduced
    clouds.  Host reads: one per ``voxel_downsample`` — two per level, source and target — for the voxel counts that
    size its results; ``register`` itself adds none."""
    from .sampling import voxel_downsample
    who = "register_pyramid"
    try:
        voxels = [float(v) for v in voxels]
    except (TypeError, ValueError):
        raise ValueError("%s: voxels must be a sequence of positive numbers" % who)
    if not voxels or not all(0 < v < float("inf") for v in voxels):
        raise ValueError("%s: voxels must be a non-empty sequence of positive finite numbers, got %r" % (who, voxels))
    if isinstance(max_dist_factor, bool) or not isinstance(max_dist_factor, numbers.Real) or not max_dist_factor > 0:
        raise ValueError("%s: max_dist_factor must be a positive number, got %r" % (who, max_dist_factor))
    if "max_dist" in kw:
        raise ValueError("%s: max_dist follows from max_dist_factor and the voxel" % who)
    normals = kw.pop("target_normals", None)
    info = kw.pop("return_info", False)
    _pair(who, source, target)
    T = init
    for level, voxel in enumerate(voxels):
        last = level == len(voxels) - 1
        src = voxel_downsample(source, voxel)[0]
        if normals is None:
            tgt, nrm = voxel_downsample(target, voxel)[0], None
        else:
            tgt, nrm = voxel_downsample(target, voxel, normals, position="point")[:2]
        T = register(src, tgt, max_dist_factor * voxel, init=T, target_normals=nrm, return_info=info and last, **kw)
    return T
