"""Point normals from the cloud itself: k-NN PCA on the GPU, and their consistent orientation.

Every path that starts from a raw cloud needs per-point normals — the cylinder and cone fits, the 6-channel network,
the evaluation entry points — and the reference only ever reads them from its data files (its own estimate_normals
call is commented out, src/utils.py:61).  ``estimate_normals`` produces them: one ``knn3_ragged`` call (fp32
difference-form neighbours, exactly ordered) and one launch of csrc/normals.hip, whose arithmetic
(csrc/normal_math.h: fp64 mean, covariance and cyclic Jacobi on the fp32 coordinates) is pinned bit for bit.

Without a viewpoint the sign is canonical (the component of largest magnitude is positive), NOT consistent over a
closed shape: that serves the cylinder fit and every other sign-invariant use.  The cone fit's axis test and the
network trained on outward normals need oriented normals.  A viewpoint the whole shape is seen from gives them for a
scan from one side; for a closed shape, which no single viewpoint sees, ``orient_normals`` (or
``estimate_normals(..., orient="mst")``) propagates the signs along the minimum spanning forest of the k-NN graph
under the weight 1 - |n_i . n_j| (Hoppe et al. 1992) and lets the topmost point of every connected component look up:
one more launch (csrc/orient.hip, definition csrc/orient_math.h), outputs exactly defined.  That kernel keeps a whole
cloud in one workgroup's LDS and stops at 10 240 points; ``engine="global"`` / ``"auto"`` runs the same definition
from global memory over many workgroups (csrc/orient_global.hip: a fixed, stream-ordered schedule of O(log n) Boruvka
rounds), the same bits on clouds of any size — a raw scan is
``estimate_normals(pts, orient="mst", search="auto", engine="auto")``.  The method's known weakness stays: the tree can
cross a sharp crease or a thin wall with the wrong sign, and an open patch gets a consistent but arbitrary side."""
import torch

from . import _lib
from . import kernels as K
from .kernels import KNN3_MAX_POINTS
from .ragged import Clouds


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


def _search(search, sizes, who):
    """The neighbour search of a call: ``search`` checked and resolved to "brute" (knn3_ragged) or "grid" (knn3_grid)."""
    if search not in (None, "grid", "auto"):
        raise ValueError("%s: search must be None, \"grid\" or \"auto\", got %r" % (who, search))
    big = bool(sizes) and max(sizes) > KNN3_MAX_POINTS
    if search is None and big:
        raise ValueError("%s: a cloud of %d points; the brute-force neighbour search takes at most %d points per cloud "
                         "(search=\"grid\" lifts the limit)" % (who, max(sizes), KNN3_MAX_POINTS))
    return "grid" if search == "grid" or (search == "auto" and big) else "brute"


def _check_engine(engine, who):
    if engine not in (None, "global", "auto"):
        raise ValueError("%s: engine must be None, \"global\" or \"auto\", got %r" % (who, engine))


def _engine(engine, sizes):
    """The orientation engine of a call (``engine`` has been checked): ``K.orient_normals`` (one workgroup per cloud;
    it raises above its limit) or ``K.orient_normals_global``."""
    if engine == "auto":
        big = bool(sizes) and max(sizes) > _lib.load().pn_orient_normals_max_points()
        return K.orient_normals_global if big else K.orient_normals
    return K.orient_normals_global if engine == "global" else K.orient_normals


def _neighbours(clouds, k, search="brute"):
    """One neighbour search over the ragged batch: idx (total,k) int32."""
    if clouds.total == 0:
        return torch.empty((0, k), dtype=torch.int32, device=clouds.flat.device)
    return (K.knn3_grid if search == "grid" else K.knn3_ragged)(clouds.flat, clouds, None, k)


def estimate_normals(points, k=16, viewpoint=None, return_scalars=False, orient=None, search=None, engine=None):
    """Normals of a cloud that has none.

    points: (N,3) or (B,N,3) fp32 on the GPU, or a list of (N_b,3) tensors (a ragged batch).
    k: neighbours per point, the point itself included, 3 .. 64.  A cloud of fewer than k points uses all of its points
       (the missing neighbours count as copies of the point); fewer than 3 points give zero normals.
    viewpoint: None — canonical sign, the component of largest magnitude positive —, or (3,), (B,3) or a list of (3,)
       tensors: the normal of point p is flipped iff n . (viewpoint - p) < 0.
    orient: None, or "mst": the canonical-sign normals are oriented consistently over every cloud as ``orient_normals``
       does, on the neighbours this call has already found — one more launch.  Not together with a viewpoint, which
       already signs every point.  Its own limit stays whatever the search: with ``engine=None`` a cloud above
       ``pn_orient_normals_max_points()`` (10 240) points is a ValueError.
    engine: only with orient="mst" — None, "global" or "auto" as in ``orient_normals``; "global" and "auto" lift the
       limit.  ``search`` and ``engine`` are independent.
    search: the neighbour search.  None — the brute-force kernel (csrc/knn3.hip), at most 10 240 points per cloud;
       "grid" — the uniform-grid search (csrc/knn3_grid.hip), the same neighbours bit for bit on clouds of any size;
       "auto" — brute force when every cloud has at most 10 240 points, the grid otherwise.  The result does not depend
       on the choice.
    Returns the normals in the layout of ``points``; with ``return_scalars`` a tuple (normals, variation, gap):
    variation = l0 / (l0 + l1 + l2) and gap = (l1 - l0) / l2 of the covariance's eigenvalues l0 <= l1 <= l2, one per
    point ((N,), (B,N) or a list).  A point whose neighbours coincide gets the zero normal and zero scalars.
    No host synchronisation and no download: the sizes come from the shapes."""
    if orient not in (None, "mst"):
        raise ValueError("estimate_normals: orient must be None or \"mst\", got %r" % (orient,))
    if orient is not None and viewpoint is not None:
        raise ValueError("estimate_normals: orient=\"mst\" together with a viewpoint (a viewpoint already signs every "
                         "point)")
    _check_engine(engine, "estimate_normals")
    if engine is not None and orient is None:
        raise ValueError("estimate_normals: engine=%r without orient=\"mst\" (the engine is the orientation's)"
                         % (engine,))
    clouds = Clouds(points, "estimate_normals")
    k = int(k)
    if not K.NORMALS_MIN_K <= k <= K.NORMALS_MAX_K:
        raise ValueError("estimate_normals: k must be %d .. %d, got %d" % (K.NORMALS_MIN_K, K.NORMALS_MAX_K, k))
    search = _search(search, clouds.sizes, "estimate_normals")
    orienter = _engine(engine, clouds.sizes) if orient == "mst" else None
    view = _viewpoints(viewpoint, clouds.S, clouds.flat.device)
    idx = _neighbours(clouds, k, search)
    out = K.point_normals(clouds.flat, clouds, idx, k, viewpoints=view, want_scalars=return_scalars)
    out = out if return_scalars else (out,)
    if orient == "mst":
        out = (orienter(clouds.flat, clouds, idx, k, out[0]),) + tuple(out[1:])
    out = tuple(clouds.per_point(o) for o in out)
    return out if return_scalars else out[0]


def orient_normals(points, normals, k=16, return_flags=False, search=None, engine=None):
    """Consistent orientation of normals without a viewpoint: spanning-tree propagation (Hoppe et al. 1992).

    points, normals: (N,3) or (B,N,3) fp32 on the GPU, or lists of (N_b,3) tensors, in the same layout; the normals may
       come from anywhere (a zero normal stays zero).
    k: neighbours per point in the graph the signs travel along, the point itself included, 1 .. 64.
    Per cloud: the minimum spanning forest of the k-NN graph under the weight 1 - |n_i . n_j| (csrc/orient_math.h fixes
    the arithmetic and a strict order on the edges, so the forest is unique); along every tree edge a normal is flipped
    iff it disagrees with its neighbour; in every connected component of the graph the point with the largest z (the
    lowest index on equal z) ends with n_z >= 0 — on a closed surface the outward normal of the topmost point is +z.
    Returns the oriented normals in the layout of ``normals`` — each the input normal or its negation, exactly; with
    ``return_flags`` a tuple (normals, flip, seed): flip 0/1 and the in-cloud index of the component's seed, int32,
    (N,), (B,N) or a list.  One neighbour search and one launch of csrc/orient.hip, no host synchronisation.
    search: None, "grid" or "auto" as in ``estimate_normals`` — the same neighbours, hence the same result.
    Limits: the tree can cross a sharp crease or a thin wall with the wrong sign; an open patch gets a consistent but
    arbitrary side.
    engine: None — the one-workgroup kernel (csrc/orient.hip); a cloud above ``pn_orient_normals_max_points()``
       (10 240) points is a ValueError.  "global" — the global-memory engine (csrc/orient_global.hip) on every cloud:
       the same definition on clouds of any size, a fixed schedule of stream-ordered launches.  "auto" — the
       one-workgroup kernel when every cloud has at most 10 240 points, the global engine for the whole call
       otherwise.  The result never depends on the engine."""
    _check_engine(engine, "orient_normals")
    clouds = Clouds(points, "orient_normals")
    n_flat = clouds.beside(normals, "orient_normals", "normals")
    if n_flat.dtype != torch.float32:
        raise ValueError("orient_normals: normals must be float32, got %s" % n_flat.dtype)
    if tuple(n_flat.shape[1:]) != (3,):
        raise ValueError("orient_normals: normals must be (N,3), (B,N,3) or a list of (N,3), got rows of %s"
                         % (tuple(n_flat.shape[1:]),))
    k = int(k)
    if not K.ORIENT_MIN_K <= k <= K.ORIENT_MAX_K:
        raise ValueError("orient_normals: k must be %d .. %d, got %d" % (K.ORIENT_MIN_K, K.ORIENT_MAX_K, k))
    search = _search(search, clouds.sizes, "orient_normals")
    orienter = _engine(engine, clouds.sizes)
    idx = _neighbours(clouds, k, search)
    out = orienter(clouds.flat, clouds, idx, k, n_flat, want_flags=return_flags)
    return tuple(clouds.per_point(o) for o in out) if return_flags else clouds.per_point(out)
