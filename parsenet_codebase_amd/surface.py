"""Trimmed surfaces of the evaluation mode: the part of the reference between the fitted parameters and the
10 000 points test.py samples off the predicted surfaces (test.py:126-168).

  * regular grids on the fitted analytic surfaces (src/primitive_forward.py:452-663: sample_plane, the second
    sample_sphere, sample_cylinder_trim, sample_cone_trim) — numpy, float64, on the downloaded parameters;
  * the occupancy of their cells (src/fitting_utils.py:240-273 create_grid) for ALL segments of a shape in one
    launch of csrc/surface.hip — or, PARSENET_TRIM_KERNEL=chamfer, by the ragged Chamfer kernel (nearest cloud point
    per cell centre, then the comparison): the same distance chain, the same masks bit for bit;
  * visualize_bit_mapping_shape (src/fitting_utils.py:713-820) -> ``trimmed_surfaces``: plain arrays
    (``TrimmedSurface``) instead of open3d meshes;
  * sample_from_collection_of_mesh (src/segment_utils.py:83-123) on the device, numpy's global stream consumed in
    the reference's order.

The one deliberate departure: sample_cone_trim trims the cone's grid PER POINT and its caller then assumes that whole
rings of 51 points survived (src/fitting_utils.py:796-797 reshapes to (len // 51, 51)).  Here a ring is kept iff its
FIRST point passes proj_min < proj < proj_max — the reference's result wherever the reference itself does not
crash or shear the grid."""
import os

import numpy as np
import torch

from . import _lib
from . import kernels as K
from ._lib import check, current_stream, h2d, ptr, require_cuda

EPS = np.finfo(np.float32).eps

# occupancy launches by the path that answered them (one per shape)
CALLS_OCCUPANCY = {"dedicated": 0, "chamfer": 0}
# the path taken when PARSENET_TRIM_KERNEL is not set.  The dedicated kernel has NOT been timed against the Chamfer path
# on an MI355X yet (tools/surface_ab.py writes profiles/surface_occupancy_ab.txt): until that record shows it faster
# it stays opt-in, like every variant here that has not won a measurement.
DEFAULT_TRIM_KERNEL = "chamfer"

_CLOSED_TYPES, _OPEN_TYPES = (0, 9, 6, 7), (2, 8)
# type -> (up-sampling rounds, default epsilon, (size_u, size_v) or None for the cone's (len / 51, 51))
_TRIM = {1: (3, 0.02, (120, 120)), 3: (3, 0.03, None), 4: (3, 0.03, (200, 60)), 5: (2, 0.03, (100, 100))}
_TRIM.update({t: (2, 0.06, (31, 30)) for t in _CLOSED_TYPES})
_TRIM.update({t: (2, 0.06, (30, 30)) for t in _OPEN_TYPES})


def trim_kernel():
    name = os.environ.get("PARSENET_TRIM_KERNEL", DEFAULT_TRIM_KERNEL)
    if name not in CALLS_OCCUPANCY:
        raise ValueError("PARSENET_TRIM_KERNEL must be one of %s, got %r" % (sorted(CALLS_OCCUPANCY), name))
    return name


class TrimmedSurface:
    """A fitted surface's regular grid and the cells the segment's points cover.
    vertices (U*V, 3) float32, row-major (vertex (i, j) is row i*size_v + j); mask (U-1, V-1) bool."""

    def __init__(self, vertices, size_u, size_v, mask):
        self.vertices = np.ascontiguousarray(vertices, dtype=np.float32).reshape(size_u * size_v, 3)
        self.size_u, self.size_v = int(size_u), int(size_v)
        self.mask = np.ascontiguousarray(mask, dtype=bool).reshape(self.size_u - 1, self.size_v - 1)

    def triangles(self):
        """(T, 3) int64 vertex indices, tessalate_points_fast's order (src/fitting_utils.py:276-295): kept cells
        row-major, (i,j),(i+1,j),(i+1,j+1) then (i,j),(i+1,j+1),(i,j+1)."""
        i, j = np.nonzero(self.mask)
        a = i.astype(np.int64) * self.size_v + j
        b = a + self.size_v
        return np.stack([a, b, b + 1, a, b + 1, a + 1], 1).reshape(-1, 3)


# ---------------------------------------------------------------------------------------
# grids on the analytic surfaces (src/primitive_forward.py:452-663), float64 like the reference
# ---------------------------------------------------------------------------------------
def sample_plane(d, n, mean):
    """:452-472: a 120 x 120 grid of half-width 0.75 around ``mean`` in the plane n.x = d; the in-plane axes come
    from two draws of numpy's global stream."""
    from .fitting import regular_parameterization
    regular_parameters = regular_parameterization(120, 120)
    n = n.reshape(3)
    r1 = np.random.random()
    r2 = np.random.random()
    a = (d - r1 * n[1] - r2 * n[2]) / (n[0] + EPS)
    x = np.array([a, r1, r2]) - d * n
    x = x / np.linalg.norm(x)
    n = n.reshape((1, 3))
    y = np.cross(x, n)
    y = y / np.linalg.norm(y)
    param = (1 - 2 * np.array(regular_parameters)) * 0.75
    return param[:, 0:1] * x + param[:, 1:2] * y + mean


def sample_sphere(radius, center):
    """:601-617 (the second, effective definition): 100 latitudes x 100 longitudes, the last longitude closing the
    circle."""
    center = center.reshape((1, 3))
    d_theta = 100
    theta = np.concatenate([np.arange(d_theta - 1) * 3.14 * 2 / d_theta, np.zeros(1)])
    circle = np.stack([np.cos(theta), np.sin(theta)], 1)
    lam = np.linspace(-1 + 1e-7, 1 - 1e-7, 100)
    radii = radius * np.sqrt(1 - lam ** 2)
    circle = np.concatenate([circle] * lam.shape[0], 0)
    new_circle = circle * np.repeat(radii, d_theta, 0).reshape((-1, 1))
    height = np.repeat(lam, d_theta, 0)
    points = np.concatenate([new_circle, height.reshape((-1, 1))], 1)
    points = points - np.mean(points, 0)
    return points + center


def sample_cylinder_trim(radius, center, axis, points):
    """:619-663: 200 heights between the extreme projections of ``points`` on the axis x 60 angles."""
    from .fitting import rotation_matrix_a_to_b
    center = center.reshape((1, 3))
    axis = axis.reshape((3, 1))
    d_theta, d_height = 60, 100
    R = rotation_matrix_a_to_b(np.array([0, 0, 1]), axis[:, 0])
    projection = (points - center) @ axis
    min_proj = np.squeeze(projection[np.argmin(projection)])
    max_proj = np.squeeze(projection[np.argmax(projection)])
    theta = np.concatenate([np.arange(d_theta - 1) * 3.14 * 2 / d_theta, np.zeros(1)])
    circle = np.stack([np.cos(theta), np.sin(theta)], 1)
    circle = np.concatenate([circle] * 2 * d_height, 0) * radius
    height = np.repeat(np.expand_dims(np.linspace(min_proj, max_proj, 2 * d_height), 1), d_theta, axis=0)
    grid = np.concatenate([circle, height], 1)
    return (R @ grid.T).T + center


def sample_cone_trim(c, a, theta, points):
    """:474-540: 100 rings of 50 angles (+ the first repeated) between the extreme projections of ``points`` on the
    axis; a ring is kept iff its first point passes the reference's per-point test (module docstring).
    Returns (R * 51, 3)."""
    c = c.reshape((3))
    a = a.reshape((3))
    norm_a = np.linalg.norm(a)
    a = a / norm_a
    proj = (points - c.reshape(1, 3)) @ a
    proj_max = np.max(proj)
    proj_min = np.min(proj)
    k = np.dot(c, a)
    x = (k - a[1] - a[2]) / (a[0] + EPS)
    d = np.array([x, 1, 1])
    p = a * (np.linalg.norm(d)) / (np.sin(theta) + EPS) * np.cos(theta) + d
    p = p.reshape((3, 1))
    Km = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    c = c.reshape((3, 1))
    a = a.reshape((3, 1))
    rel_unit_vector = (p - c) / np.linalg.norm(p - c)
    rel_unit_vector_min = rel_unit_vector * (proj_min) / (np.cos(theta) + EPS)
    rel_unit_vector_max = rel_unit_vector * (proj_max) / (np.cos(theta) + EPS)
    degrees = 2 * np.pi * 0.01 * np.arange(50) * 2
    R = np.stack([np.eye(3) + np.sin(g) * Km + (1 - np.cos(g)) * Km @ Km for g in degrees], 0)     # (50,3,3)
    p_ = np.stack([rel_unit_vector_min + (rel_unit_vector_max - rel_unit_vector_min) * 0.01 * j
                   for j in range(100)], 0)                                                        # (100,3,1)
    rings = (R[None] @ p_[:, None])[..., 0] + c.reshape((1, 1, 3))                                 # (100,50,3)
    rings = np.concatenate([rings, rings[:, 0:1]], 1)                                              # (100,51,3)
    first = ((rings[:, 0] - c.reshape((1, 3))) @ a)[:, 0]
    keep = np.logical_and(first < proj_max, first > proj_min)
    return rings[keep].reshape(-1, 3)


# ---------------------------------------------------------------------------------------
# occupancy of the grid cells
# ---------------------------------------------------------------------------------------
def cell_centres(grid, size_u, size_v):
    """The pinned tensor expression: (((v[i][j] + v[i][j+1]) + v[i+1][j]) + v[i+1][j+1]) * 0.25, fp32."""
    g = grid.reshape(size_u, size_v, 3)
    return ((((g[:-1, :-1] + g[:-1, 1:]) + g[1:, :-1]) + g[1:, 1:]) * 0.25).reshape(-1, 3)


def grid_occupancy(grids, sizes, clouds, thres, kernel=None):
    """Segment s: grid grids[s] (U*V, 3) with sizes[s] = (U, V), cloud clouds[s] (P, 3), threshold thres[s]; fp32
    tensors on the GPU.  Returns the list of (U-1, V-1) bool masks (on the GPU): a cell is kept iff
    sqrt(min_p |centre - p|^2) < thres, fp32, the distance chain of the Chamfer kernel.  ONE launch."""
    kernel = kernel or trim_kernel()
    if kernel not in CALLS_OCCUPANCY:
        raise ValueError("unknown occupancy kernel %r" % (kernel,))
    S = len(grids)
    if S == 0:
        return []
    require_cuda(*grids)
    require_cuda(*clouds)
    dev = grids[0].device
    for g, (u, v), c in zip(grids, sizes, clouds):
        if u < 2 or v < 2 or g.shape[0] != u * v:
            raise ValueError("grid_occupancy: a %s grid with sizes %s" % (tuple(g.shape), (u, v)))
        if c.shape[0] < 1:
            raise ValueError("grid_occupancy: empty cloud")
    ncell = np.asarray([(u - 1) * (v - 1) for u, v in sizes], np.int64)
    cell_off = np.concatenate([[0], np.cumsum(ncell)])
    coff = np.concatenate([[0], np.cumsum([c.shape[0] for c in clouds])])
    cloud = torch.cat([c.reshape(-1, 3) for c in clouds]).float().contiguous()
    thr = np.asarray(thres, np.float32)
    CALLS_OCCUPANCY[kernel] += 1
    if kernel == "chamfer":
        centres = torch.cat([cell_centres(g.float(), u, v) for g, (u, v) in zip(grids, sizes)]).contiguous()
        table = h2d(np.concatenate([cell_off, coff]).astype(np.int32), dev)
        minA = K.chamfer_nn_ragged(centres, table[:S + 1], int(ncell.max()), cloud, table[S + 1:],
                                   int(np.diff(coff).max()), True, False)[0]
        flat = torch.sqrt(minA) < h2d(np.repeat(thr, ncell), dev)
    else:
        voff = np.concatenate([[0], np.cumsum([u * v for u, v in sizes])])
        if max(voff[-1], coff[-1]) * 3 >= 2 ** 31:
            raise ValueError("grid_occupancy: int32 offsets")
        grid = torch.cat([g.reshape(-1, 3) for g in grids]).float().contiguous()
        lib = _lib.load()
        tile = lib.pn_grid_occupancy_tile()
        tile_off = np.concatenate([[0], np.cumsum((ncell + tile - 1) // tile)])
        su = np.asarray([u for u, _ in sizes])
        sv = np.asarray([v for _, v in sizes])
        table = h2d(np.concatenate([su, sv, voff[:S], coff, tile_off, cell_off[:S], thr.view(np.int32)])
                    .astype(np.int32), dev)
        o = np.cumsum([0, S, S, S, S + 1, S + 1, S])
        col = [table[o[i]:o[i + 1] if i + 1 < len(o) else None] for i in range(len(o))]
        flat = torch.empty(int(cell_off[-1]), dtype=torch.uint8, device=dev)
        with _lib.on_device(dev):
            rc = lib.pn_grid_occupancy_ragged_f32(ptr(grid), ptr(col[0]), ptr(col[1]), ptr(col[2]), ptr(cloud),
                                                  ptr(col[3]), ptr(col[6]), ptr(col[4]), ptr(col[5]), S,
                                                  int(tile_off[-1]), ptr(flat), current_stream(dev))
        check(rc, "pn_grid_occupancy_ragged_f32")
        flat = flat.bool()
    return [flat[cell_off[s]:cell_off[s + 1]].reshape(sizes[s][0] - 1, sizes[s][1] - 1) for s in range(S)]


def _as_numpy(x):
    return x if isinstance(x, np.ndarray) else x.detach().cpu().numpy()


def bit_mapping_points_torch(input, output_points, thres, size_u, size_v, mesh=None):
    """src/fitting_utils.py:663-667 for one segment: -> TrimmedSurface."""
    dev = input.device if torch.is_tensor(input) and input.is_cuda else torch.device("cuda", torch.cuda.current_device())
    grid = torch.as_tensor(_as_numpy(output_points).astype(np.float32)).reshape(-1, 3)
    cloud = input if torch.is_tensor(input) else torch.as_tensor(np.asarray(input).astype(np.float32))
    mask = grid_occupancy([grid.to(dev)], [(size_u, size_v)], [cloud.float().to(dev)], [thres])[0]
    return TrimmedSurface(grid.numpy(), size_u, size_v, mask.cpu().numpy())


def trimmed_surfaces(data, recon_points, epsilon=None):
    """src/fitting_utils.py:713-820 (visualize_bit_mapping_shape with bit_map=True): for every segment with a
    reconstruction, the segment's points up-sampled (x4, analytic surfaces other than the sphere x8), the grid of
    its fitted surface and the cells with a point of the up-sampled cloud within epsilon (default per type: closed
    and open splines 0.06, plane 0.02, others 0.03).  ``data``: the rows fit_one_shape_torch takes;
    ``recon_points``: its second result.  All segments go through ONE occupancy launch.  -> [TrimmedSurface]."""
    from .fitting import up_sample_points_torch_memory_efficient
    grids, sizes, clouds, thres, host = [], [], [], [], []
    for g, rec in zip(data, recon_points):
        if rec is None or (isinstance(rec, np.ndarray) and rec.shape[0] == 0):
            continue            # degenerate segments
        seg_type = int(g[2])
        if seg_type not in _TRIM:
            raise ValueError("trimmed_surfaces: no grid for primitive type %r" % (seg_type,))
        rounds, eps_default, size = _TRIM[seg_type]
        pts = g[0]
        if not torch.is_tensor(pts):
            pts = torch.from_numpy(np.asarray(pts, np.float32))
        pts = pts.float().cuda()
        if torch.is_tensor(rec):                      # spline samples (1, U*V, 3) on the device
            rec = rec.detach()[0].float()
            grid_host = rec.cpu().numpy()
        else:
            grid_host = np.asarray(rec).astype(np.float32)
            rec = h2d(grid_host, pts.device)
        if size is None:
            size = (grid_host.shape[0] // 51, 51)
        if size[0] < 2 or grid_host.shape[0] != size[0] * size[1]:
            continue            # (a cone whose trimming left fewer than two rings: nothing to tessellate)
        grids.append(rec.reshape(-1, 3))
        sizes.append(size)
        clouds.append(up_sample_points_torch_memory_efficient(pts, rounds))
        thres.append(epsilon if epsilon else eps_default)
        host.append(grid_host)
    masks = grid_occupancy(grids, sizes, clouds, thres)
    if not masks:
        return []
    flat = torch.cat([m.reshape(-1) for m in masks]).cpu().numpy()       # one download
    out, o = [], 0
    for gh, (u, v) in zip(host, sizes):
        n = (u - 1) * (v - 1)
        out.append(TrimmedSurface(gh, u, v, flat[o:o + n]))
        o += n
    return out


def visualize_bit_mapping_shape(data_, weights, recon_points, parameters=None, bit_map=True, epsilon=0.05):
    """The reference's name and argument order (src/fitting_utils.py:713)."""
    if not bit_map:
        raise NotImplementedError("visualize_bit_mapping_shape(bit_map=False): untrimmed meshes are viewer output")
    return trimmed_surfaces(data_, recon_points, epsilon)


# ---------------------------------------------------------------------------------------
# area-weighted samples of a collection of trimmed surfaces (src/segment_utils.py:83-123)
# ---------------------------------------------------------------------------------------
def _mesh_tables(surfaces, dev):
    """Grids, kept cells and face offsets of the surfaces on the device."""
    M = len(surfaces)
    voff = np.concatenate([[0], np.cumsum([s.vertices.shape[0] for s in surfaces])])
    cells = [np.nonzero(s.mask.reshape(-1))[0] for s in surfaces]
    face_off = np.concatenate([[0], np.cumsum([2 * c.shape[0] for c in cells])])
    grid = h2d(np.concatenate([s.vertices for s in surfaces]), dev)
    table = h2d(np.concatenate([voff[:M], [s.size_v for s in surfaces], face_off, np.concatenate(cells)])
                .astype(np.int32), dev)
    return grid, table[:M], table[M:2 * M], table[2 * M:3 * M + 1], table[3 * M + 1:], face_off


def triangle_areas(surfaces, device=None):
    """Per surface the float64 areas of its triangles (src/utils.py:174-178 on the widened fp32 vertices), on the
    GPU.  Surfaces must have a kept cell."""
    dev = device or torch.device("cuda", torch.cuda.current_device())
    grid, voff, sv, foff, cells, face_off = _mesh_tables(surfaces, dev)
    area = torch.empty(int(face_off[-1]), dtype=torch.float64, device=dev)
    with _lib.on_device(dev):
        rc = _lib.load().pn_trimesh_area_f64(ptr(grid), ptr(voff), ptr(sv), ptr(foff), ptr(cells), len(surfaces),
                                             int(face_off[-1]), ptr(area), current_stream(dev))
    check(rc, "pn_trimesh_area_f64")
    return [area[face_off[m]:face_off[m + 1]] for m in range(len(surfaces))]


def sample_counts(areas, N):
    """n_i = int((N * A_i) // sum A); only meshes with n_i > 10 are sampled (others get 0)."""
    A = [float(a) for a in areas]
    total = np.sum(A)
    n = [int((N * a) // total) for a in A]
    return [k if k > 10 else 0 for k in n]


def sample_draws(counts):
    """Per sampled surface the uniforms of sample_mesh, in its order: the face picks (random.choice draws
    random_sample(n)), then u = rand(n, 1), then v = rand(n, 1) — numpy's global stream."""
    return [(np.random.random_sample(k), np.random.rand(k, 1)[:, 0], np.random.rand(k, 1)[:, 0]) for k in counts]


def sample_from_collection_of_mesh(Meshes, N=10000, return_faces=False):
    """src/segment_utils.py:83-123: N points over all trimmed surfaces, shared out by area.  Surfaces without a kept
    cell are dropped; surface i gets n_i = int((N * A_i) // sum A) points and is sampled only if n_i > 10
    (sample_mesh, src/utils.py:123-154: face by area + min area + 1e-10, uniform barycentric coordinates); per
    sampled surface numpy's global stream gives random_sample(n_i), rand(n_i, 1), rand(n_i, 1) in that order.
    Returns float32 (sum n_i, 3) (numpy); ``return_faces``: also the list of the face ids taken per sampled
    surface."""
    dev = torch.device("cuda", torch.cuda.current_device())
    meshes = [m for m in Meshes if m.mask.any()]
    if not meshes:
        raise ValueError("sample_from_collection_of_mesh: no surface with a kept cell")
    areas = triangle_areas(meshes, dev)
    A = torch.stack([a.sum() for a in areas]).cpu().numpy()
    counts = sample_counts(A, N)
    take = [i for i, k in enumerate(counts) if k > 0]
    if not take:
        raise ValueError("sample_from_collection_of_mesh: no surface gets more than 10 of the %d points" % N)
    draws = sample_draws([counts[i] for i in take])
    sampled = [meshes[i] for i in take]
    cdf = []
    for i in take:
        a = areas[i]
        a = a + torch.min(a) + 1e-10
        c = torch.cumsum(a / torch.sum(a), 0)
        cdf.append(c / c[-1])
    grid, voff, sv, foff, cells, face_off = _mesh_tables(sampled, dev)
    samp_off = np.concatenate([[0], np.cumsum([counts[i] for i in take])])
    total = int(samp_off[-1])
    uni = h2d(np.concatenate([np.concatenate([d[j] for d in draws]) for j in range(3)]), dev)
    soff = h2d(samp_off.astype(np.int32), dev)
    cdf = torch.cat(cdf).contiguous()
    out = torch.empty(total, 3, dtype=torch.float32, device=dev)
    face = torch.empty(total, dtype=torch.int32, device=dev) if return_faces else None
    with _lib.on_device(dev):
        rc = _lib.load().pn_trimesh_sample_f64(ptr(grid), ptr(voff), ptr(sv), ptr(foff), ptr(cells), ptr(cdf), ptr(soff),
                                               ptr(uni[:total]), ptr(uni[total:2 * total]), ptr(uni[2 * total:]),
                                               len(sampled), total, ptr(out), ptr(face), current_stream(dev))
    check(rc, "pn_trimesh_sample_f64")
    points = out.cpu().numpy()
    if return_faces:
        f = face.cpu().numpy()
        return points, [f[samp_off[i]:samp_off[i + 1]] for i in range(len(take))]
    return points


# ---------------------------------------------------------------------------------------
# exact distance from points to the trimmed surfaces (csrc/tridist.hip)
# ---------------------------------------------------------------------------------------
# launches of point_surface_distance (one of each per call, whatever the batch)
CALLS_TRIDIST = {"records": 0, "distance": 0}
# the last pruned call: "skipped" a one-element int64 tensor on the device (groups of triangles the waves skipped;
# reading it synchronises), "visits" the number of (wave, group) pairs an unpruned call walks
LAST_PRUNE = {"skipped": None, "visits": 0}


def _tridist_args(points_list, surfaces_list):
    """Host-only argument checks of point_surface_distance -> per shape the positions of the surfaces with a kept
    cell.  ValueError names the shape."""
    if len(points_list) != len(surfaces_list) or len(points_list) < 1:
        raise ValueError("point_surface_distance: %d point clouds for %d lists of surfaces"
                         % (len(points_list), len(surfaces_list)))
    kept = []
    for b, (p, surfaces) in enumerate(zip(points_list, surfaces_list)):
        shape = tuple(p.shape) if hasattr(p, "shape") else np.asarray(p).shape
        if len(shape) != 2 or shape[1] != 3 or shape[0] < 1:
            raise ValueError("point_surface_distance: shape %d: points must be (N,3) with N >= 1, got %s"
                             % (b, tuple(shape)))
        pos = [i for i, s in enumerate(surfaces) if s.mask.any()]
        if not pos:
            raise ValueError("point_surface_distance: shape %d has no kept triangle (%d surfaces, none with a kept "
                             "cell)" % (b, len(surfaces)))
        kept.append(pos)
    return kept


def _morton_order(points, shape_of_row):
    """Rows ordered shape by shape and, inside a shape, along a 30-bit Morton curve through the batch's bounding box:
    the 64 points of a wave are then neighbours, which is what lets a wave skip a group of triangles.  The order has
    no influence on any result (a point's result depends on the point alone)."""
    lo = points.min(0).values
    span = (points.max(0).values - lo).clamp_min(1e-30)
    q = ((points - lo) / span * 1023.0).to(torch.int64).clamp_(0, 1023)
    q = (q | (q << 16)) & 0x30000FF
    q = (q | (q << 8)) & 0x300F00F
    q = (q | (q << 4)) & 0x30C30C3
    q = (q | (q << 2)) & 0x9249249
    code = q[:, 0] | (q[:, 1] << 1) | (q[:, 2] << 2) | (shape_of_row << 30)
    return torch.argsort(code)


def point_surface_distance(points_list, surfaces_list, prune=True, return_index=False, waves=None):
    """Per shape the (N_b,) float32 SQUARED distance from every point to the nearest triangle of the kept cells of
    the shape's trimmed surfaces — the surface itself, not samples of it.  points_list[b]: (N_b,3) array or tensor;
    surfaces_list[b]: a list of TrimmedSurface (those without a kept cell are skipped; a shape left with none raises
    ValueError naming it).  ``return_index``: per shape (d2, surface, face) with the position of the nearest surface
    in surfaces_list[b] and the face id within it (TrimmedSurface.triangles() order), int64, the lowest on equal
    distances.  ``prune`` skips groups of triangles by a certified bound; results are bit-identical with it on and
    off.  ``waves`` (4, 8, 16; default by the number of point tiles) is the workgroup size of the distance pass and
    has no influence on the results either.  ONE record launch and ONE distance launch for the whole batch."""
    kept = _tridist_args(points_list, surfaces_list)
    B = len(kept)
    dev = torch.device("cuda", torch.cuda.current_device())
    pts = [torch.from_numpy(np.asarray(p, np.float32)).to(dev) if not torch.is_tensor(p)
           else p.detach().to(device=dev, dtype=torch.float32) for p in points_list]
    flat = [surfaces_list[b][i] for b in range(B) for i in kept[b]]
    grid, voff, sv, foff, cells, face_off = _mesh_tables(flat, dev)
    lib = _lib.load()
    group, tile = lib.pn_trimesh_group(), lib.pn_trimesh_point_dist_tile()
    mesh_off = np.concatenate([[0], np.cumsum([len(k) for k in kept])])
    shape_face = face_off[mesh_off]
    slots = (np.diff(shape_face) + group - 1) // group * group
    slot_off = np.concatenate([[0], np.cumsum(slots)])
    counts = np.asarray([p.shape[0] for p in pts], np.int64)
    pt_off = np.concatenate([[0], np.cumsum(counts)])
    total_slots, T = int(slot_off[-1]), int(pt_off[-1])
    if max(3 * T, 16 * total_slots, 3 * grid.shape[0]) >= 2 ** 31:
        raise ValueError("point_surface_distance: int32 offsets")
    ntile = (counts + tile - 1) // tile
    tile_shape = np.repeat(np.arange(B), ntile)
    tile_first = np.concatenate([pt_off[b] + tile * np.arange(ntile[b]) for b in range(B)])
    total_tiles = int(ntile.sum())
    if waves is None:
        waves = 16 if total_tiles <= 256 else 8 if total_tiles <= 512 else 4
    table = h2d(np.concatenate([shape_face, slot_off, pt_off, tile_shape, tile_first]).astype(np.int32), dev)
    o = np.cumsum([0, B + 1, B + 1, B + 1, total_tiles])
    c_face, c_slot, c_pt, c_tshape, c_tfirst = [table[o[i]:o[i + 1] if i + 1 < len(o) else None]
                                                 for i in range(len(o))]
    rec = torch.empty(16 * total_slots, dtype=torch.float32, device=dev)
    sph = torch.empty(total_slots // group, 4, dtype=torch.float32, device=dev)
    allp = (pts[0] if B == 1 else torch.cat(pts)).contiguous()
    order = None
    if prune:
        order = _morton_order(allp, h2d(np.repeat(np.arange(B), counts), dev))
        allp = allp[order].contiguous()
    d2 = torch.empty(T, dtype=torch.float32, device=dev)
    face = torch.empty(T, dtype=torch.int32, device=dev)
    skipped = torch.zeros(1, dtype=torch.int64, device=dev) if prune else None
    with _lib.on_device(dev):
        stream = current_stream(dev)
        rc = lib.pn_trimesh_records_f32(ptr(grid), ptr(voff), ptr(sv), ptr(foff), ptr(cells), len(flat), ptr(c_face),
                                        ptr(c_slot), B, total_slots, ptr(rec), ptr(sph), stream)
        check(rc, "pn_trimesh_records_f32")
        CALLS_TRIDIST["records"] += 1
        rc = lib.pn_trimesh_point_dist_f32(ptr(allp), ptr(c_pt), ptr(c_slot), ptr(rec), total_slots, ptr(sph),
                                           ptr(c_tshape), ptr(c_tfirst), B, total_tiles, int(waves),
                                           1 if prune else 0, ptr(d2), ptr(face), ptr(skipped), stream)
        check(rc, "pn_trimesh_point_dist_f32")
        CALLS_TRIDIST["distance"] += 1
    if prune:
        LAST_PRUNE["skipped"] = skipped
        LAST_PRUNE["visits"] = int((ntile * (slots // group)).sum())
        d2 = torch.empty_like(d2).index_copy_(0, order, d2)
        face = torch.empty_like(face).index_copy_(0, order, face)
    out = []
    for b in range(B):
        # own storage per shape: what a caller reduces must not depend on the batch the shape was evaluated in
        d = d2[pt_off[b]:pt_off[b + 1]].clone()
        if not return_index:
            out.append(d)
            continue
        f = face[pt_off[b]:pt_off[b + 1]].long()
        local = face_off[mesh_off[b]:mesh_off[b + 1] + 1] - face_off[mesh_off[b]]
        m = torch.searchsorted(h2d(local[1:].astype(np.int64), dev), f, right=True)
        out.append((d, h2d(np.asarray(kept[b], np.int64), dev)[m], f - h2d(local.astype(np.int64), dev)[m]))
    return out
