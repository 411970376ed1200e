"""Point normals from the cloud itself: k-NN PCA on the GPU.

Every path that starts from a raw cloud needs per-point normals — the cylinder and cone fits, the 6-channel network,
the evaluation entry points — and the reference only ever reads them from its data files (its own estimate_normals
call is commented out, src/utils.py:61).  ``estimate_normals`` produces them: one ``knn3_ragged`` call (fp32
difference-form neighbours, exactly ordered) and one launch of csrc/normals.hip, whose arithmetic
(csrc/normal_math.h: fp64 mean, covariance and cyclic Jacobi on the fp32 coordinates) is pinned bit for bit.

Without a viewpoint the sign is canonical (the component of largest magnitude is positive), NOT consistent over a
closed shape: that serves the cylinder fit and every other sign-invariant use.  The cone fit's axis test and the
network trained on outward normals need oriented normals, i.e. a viewpoint the whole shape is seen from."""
import numpy as np
import torch

from . import _lib
from . import kernels as K

KNN3_MAX_POINTS = 10240      # pn_knn3_ragged's limit on the points of one segment (fp32 mode)


def _viewpoints(viewpoint, S, device):
    """None, (3,), (S,3) or a list of S (3,) tensors -> (S,3) fp32 on the device, or None."""
    if viewpoint is None:
        return None
    if isinstance(viewpoint, (list, tuple)):
        if len(viewpoint) != S or not all(torch.is_tensor(v) and tuple(v.shape) == (3,) for v in viewpoint):
            raise ValueError("estimate_normals: a list of viewpoints holds one (3,) tensor per cloud (%d)" % S)
        _lib.require_cuda(*viewpoint)
        viewpoint = torch.stack(list(viewpoint))
    if not torch.is_tensor(viewpoint):
        raise TypeError("estimate_normals: viewpoint must be None, a tensor or a list of tensors")
    _lib.require_cuda(viewpoint)
    if viewpoint.dtype != torch.float32:
        raise ValueError("estimate_normals: viewpoint must be float32, got %s" % viewpoint.dtype)
    if tuple(viewpoint.shape) == (3,):
        viewpoint = viewpoint.reshape(1, 3).expand(S, 3)
    if tuple(viewpoint.shape) != (S, 3):
        raise ValueError("estimate_normals: viewpoint must be (3,) or (%d,3), got %s" % (S, tuple(viewpoint.shape)))
    return viewpoint.to(device).contiguous()


def estimate_normals(points, k=16, viewpoint=None, return_scalars=False):
    """Normals of a cloud that has none.

    points: (N,3) or (B,N,3) fp32 on the GPU, or a list of (N_b,3) tensors (a ragged batch).
    k: neighbours per point, the point itself included, 3 .. 64.  A cloud of fewer than k points uses all of its points
       (the missing neighbours count as copies of the point); fewer than 3 points give zero normals.
    viewpoint: None — canonical sign, the component of largest magnitude positive —, or (3,), (B,3) or a list of (3,)
       tensors: the normal of point p is flipped iff n . (viewpoint - p) < 0.
    Returns the normals in the layout of ``points``; with ``return_scalars`` a tuple (normals, variation, gap):
    variation = l0 / (l0 + l1 + l2) and gap = (l1 - l0) / l2 of the covariance's eigenvalues l0 <= l1 <= l2, one per
    point ((N,), (B,N) or a list).  A point whose neighbours coincide gets the zero normal and zero scalars.
    No host synchronisation and no download: the sizes come from the shapes."""
    if isinstance(points, (list, tuple)):
        clouds = list(points)
        if not clouds:
            raise ValueError("estimate_normals: an empty list of clouds")
        if not all(torch.is_tensor(c) for c in clouds):
            raise TypeError("estimate_normals: a list of clouds holds tensors")
        layout = "list"
    elif torch.is_tensor(points):
        clouds = [points]
        layout = "single" if points.dim() == 2 else "batch"
    else:
        raise TypeError("estimate_normals: points must be a tensor or a list of tensors")
    _lib.require_cuda(*clouds)
    for c in clouds:
        if c.dtype != torch.float32:
            raise ValueError("estimate_normals: points must be float32, got %s" % c.dtype)
        if c.dim() != (3 if layout == "batch" else 2) or c.shape[-1] != 3:
            raise ValueError("estimate_normals: points must be (N,3), (B,N,3) or a list of (N,3), got %s"
                             % (tuple(c.shape),))
    k = int(k)
    if not K.NORMALS_MIN_K <= k <= K.NORMALS_MAX_K:
        raise ValueError("estimate_normals: k must be %d .. %d, got %d" % (K.NORMALS_MIN_K, K.NORMALS_MAX_K, k))
    if layout == "batch":
        B, N = points.shape[:2]
        sizes = [N] * B
        flat = points.reshape(B * N, 3)
    else:
        sizes = [c.shape[0] for c in clouds]
        flat = clouds[0] if len(clouds) == 1 else torch.cat(clouds)
    if sizes and max(sizes) > KNN3_MAX_POINTS:
        raise ValueError("estimate_normals: a cloud of %d points; the neighbour search takes at most %d points per "
                         "cloud" % (max(sizes), KNN3_MAX_POINTS))
    S = len(sizes)
    dev = flat.device
    view = _viewpoints(viewpoint, S, dev)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    total = int(off[-1])
    if total == 0:
        idx = torch.empty((0, k), dtype=torch.int32, device=dev)
    else:
        idx = K.knn3_ragged(flat, _lib.h2d(off.astype(np.int32), dev), max(sizes), k)
    out = K.point_normals(flat, off, idx, k, viewpoints=view, want_scalars=return_scalars)
    out = out if return_scalars else (out,)
    if layout == "batch":
        out = (out[0].reshape(B, N, 3),) + tuple(o.reshape(B, N) for o in out[1:])
    elif layout == "list":
        out = tuple(list(torch.split(o, sizes)) for o in out)
    return tuple(out) if return_scalars else out[0]
