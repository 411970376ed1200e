"""CPU-side checks of the dominant-plane extraction: csrc/plane_math.h compiled for the host into a serial simulation of
the kernels' schedule (tests/native/plane_host.cpp: bounds, hypotheses, scores per tile with a flush of the tile's
counters, selection, the refinement rounds over the tree of csrc/outlier_math.h, inlier and dist) against ``plane_numpy``,
an independent numpy / Python restatement of the definition (the hash in Python integers, planes and distances as
elementwise fp64 numpy, the tree sums of tests/test_outlier_abi.py, the Jacobi in Python floats) — every output equal
bit for bit, with both orders of arrival —, the exact properties of the definition, the stand-alone program under the
address and undefined-behaviour sanitizers, the exports of csrc/plane.hip, their schedule, workspace and argument checks."""
import ctypes
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests.helpers import native
from tests.test_fps_abi import same
from tests.test_knn3_grid_abi import collinear, copies_among_random, identical, lattice, offset_cloud, planar
from tests.test_outlier_abi import tree_sum
from tests.test_point_normals_abi import BAR, GAP_MIN

SOURCE = native.source("plane_host.cpp")
NAMES = ("pn_plane_f32", "pn_plane_workspace_bytes", "pn_plane_launches")
M64 = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15
SWEEPS = 5           # NM_SWEEPS of csrc/normal_math.h   (test_the_constants_are_the_ones_the_tests_assume)
TINY = 1e-30         # NM_TINY
CHUNK = 256          # hypotheses scored at a time


# ---------------------------------------------------------------------------------------------
# the definition, in numpy and Python (shared with tests/test_plane_gpu.py)
# ---------------------------------------------------------------------------------------------
def mix(z):
    """The splitmix64 finaliser on a Python integer below 2^64."""
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draws(seed, H, n):
    """(H,3) int64: the three indices of every hypothesis."""
    seed &= M64
    return np.asarray([[((mix((seed + GOLD * (3 * h + s + 1)) & M64) >> 32) * n) >> 32 for s in range(3)]
                       for h in range(H)], np.int64).reshape(H, 3)


def unit_axis(axis):
    """The axis as the host normalises it: a / sqrt((ax ax + ay ay) + az az) in fp64."""
    a = np.asarray(axis, np.float64)
    return a / np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])


def min_cos_of(max_angle):
    return min(1.0, max(0.0, math.cos(math.radians(float(max_angle)))))


def canonical(nx, ny, nz):
    """The component of largest magnitude positive, the lowest axis on a tie (arrays or scalars)."""
    ax, ay, az = np.abs(nx), np.abs(ny), np.abs(nz)
    lead = np.where((ax >= ay) & (ax >= az), nx, np.where(ay >= az, ny, nz))
    flip = lead < 0
    return np.where(flip, -nx, nx), np.where(flip, -ny, ny), np.where(flip, -nz, nz)


def dot3(nx, ny, nz, x, y, z):
    """(nx x + ny y) + nz z, one rounding per operation."""
    a = nx * x
    b = ny * y
    a = a + b
    b = nz * z
    return a + b


def hypotheses_numpy(X, idx, axis, min_cos):
    """X (n,3) fp64, idx (H,3) -> (q (H,4) fp64, valid (H) bool)."""
    with np.errstate(all="ignore"):
        p0, p1, p2 = X[idx[:, 0]], X[idx[:, 1]], X[idx[:, 2]]
        a, b = p1 - p0, p2 - p0
        cx = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
        cy = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
        cz = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
        len2 = (cx * cx + cy * cy) + cz * cz
        valid = (idx[:, 0] != idx[:, 1]) & (idx[:, 0] != idx[:, 2]) & (idx[:, 1] != idx[:, 2])
        valid &= (len2 > 0) & np.isfinite(len2)
        length = np.sqrt(len2)
        nx, ny, nz = canonical(cx / length, cy / length, cz / length)
        d = -dot3(nx, ny, nz, p0[:, 0], p0[:, 1], p0[:, 2])
        if axis is not None:
            valid &= np.abs(dot3(nx, ny, nz, axis[0], axis[1], axis[2])) >= min_cos
    return np.stack([nx, ny, nz, d], 1), valid


def signed_numpy(q, X):
    """q (...,4) against X (n,3) -> (..., n) fp64: ((nx x + ny y) + nz z) + d."""
    q = np.asarray(q, np.float64)
    with np.errstate(all="ignore"):
        s = dot3(q[..., 0, None], q[..., 1, None], q[..., 2, None], X[:, 0], X[:, 1], X[:, 2])
        return s + q[..., 3, None]


def jacobi_python(a00, a01, a02, a11, a12, a22):
    """The cyclic Jacobi of csrc/normal_math.h in Python floats -> (A, V): the rotated matrix and the columns."""
    A = [[a00, a01, a02], [a01, a11, a12], [a02, a12, a22]]
    V = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for _ in range(SWEEPS):
        for p, q, r in ((0, 1, 2), (0, 2, 1), (1, 2, 0)):
            apq = A[p][q]
            if apq == 0.0:
                continue
            theta = (A[q][q] - A[p][p]) / (2.0 * apq)
            at = 1.0 / (abs(theta) + math.sqrt(theta * theta + 1.0))
            t = -at if theta < 0.0 else at
            c = 1.0 / math.sqrt(t * t + 1.0)
            s = t * c
            A[p][p] = A[p][p] - t * apq
            A[q][q] = A[q][q] + t * apq
            A[p][q] = A[q][p] = 0.0
            arp, arq = A[r][p], A[r][q]
            A[r][p] = A[p][r] = c * arp - s * arq
            A[r][q] = A[q][r] = s * arp + c * arq
            for k in range(3):
                vp, vq = V[k][p], V[k][q]
                V[k][p] = c * vp - s * vq
                V[k][q] = s * vp + c * vq
    return A, V


def refit_python(mean, sums, m, axis, min_cos):
    """The refit of a round from the mean (3), the six moment sums and the count -> (nx, ny, nz, d) or None."""
    if m < 3:
        return None
    dm = float(m)
    a = [float(s) / dm for s in sums]
    A, V = jacobi_python(*a)
    l0, col = A[0][0], 0
    if A[1][1] < l0:
        l0, col = A[1][1], 1
    if A[2][2] < l0:
        l0, col = A[2][2], 2
    hi01 = A[1][1] if A[0][0] < A[1][1] else A[0][0]
    l2 = A[2][2] if hi01 < A[2][2] else hi01
    if not l2 > TINY:
        return None
    nx, ny, nz = V[0][col], V[1][col], V[2][col]
    length = math.sqrt((nx * nx + ny * ny) + nz * nz)
    nx, ny, nz = (float(v) for v in canonical(np.float64(nx / length), np.float64(ny / length),
                                               np.float64(nz / length)))
    if axis is not None and not abs((nx * float(axis[0]) + ny * float(axis[1])) + nz * float(axis[2])) >= min_cos:
        return None
    mx, my, mz = (float(v) for v in mean)
    return nx, ny, nz, -((nx * mx + ny * my) + nz * mz)


def threshold_status(t):
    t = np.float32(t)
    return 0 if (t > 0 and np.isfinite(t)) else -2


def plane_numpy(P, t, H, seed, refine, axis=None, min_cos=0.0):
    """One cloud by the definition -> a dict: plane (4) fp64, count, best, inlier (n) uint8, dist (n) fp32, dist64 (n)
    fp64 (what dist is the rounding of), valid (H) bool (the hypotheses)."""
    P = np.ascontiguousarray(P, np.float32).reshape(-1, 3)
    n = P.shape[0]
    X = P.astype(np.float64)
    t64 = np.float64(np.float32(t))
    out = dict(plane=np.zeros(4), count=0, best=-1, inlier=np.zeros(n, np.uint8), dist=np.full(n, np.nan, np.float32),
               dist64=np.full(n, np.nan), valid=np.zeros(H, bool))
    status = -1 if not np.isfinite(P).all() else threshold_status(t)
    if n >= 3:
        q, out["valid"] = hypotheses_numpy(X, draws(seed, H, n), axis, min_cos)
    if status:
        out["count"] = status
        return out
    if n < 3 or not out["valid"].any():
        return out
    valid = out["valid"]
    counts = np.zeros(H, np.int64)
    for h0 in range(0, H, CHUNK):
        with np.errstate(invalid="ignore"):
            counts[h0:h0 + CHUNK] = (np.abs(signed_numpy(q[h0:h0 + CHUNK], X)) <= t64).sum(1)
    key = max((int(counts[h]) << 32) | (0xFFFFFFFF - h) for h in range(H) if valid[h])
    best, count = 0xFFFFFFFF - (key & 0xFFFFFFFF), key >> 32
    plane = q[best].copy()
    for _ in range(refine):
        inl = np.abs(signed_numpy(plane, X)) <= t64
        mean = [tree_sum(np.where(inl, X[:, a], 0.0)) / np.float64(count) for a in range(3)]
        dx, dy, dz = X[:, 0] - mean[0], X[:, 1] - mean[1], X[:, 2] - mean[2]
        with np.errstate(over="ignore", invalid="ignore"):
            sums = [tree_sum(np.where(inl, u * v, 0.0)) for u, v in ((dx, dx), (dx, dy), (dx, dz), (dy, dy), (dy, dz),
                                                                      (dz, dz))]
        cand = refit_python(mean, sums, count, axis, min_cos)
        if cand is None:
            break
        cand = np.asarray(cand, np.float64)
        m = int((np.abs(signed_numpy(cand, X)) <= t64).sum())
        if m < count:
            break
        plane, count = cand, m
    s = signed_numpy(plane, X)
    out.update(plane=plane, count=int(count), best=int(best), inlier=(np.abs(s) <= t64).astype(np.uint8),
               dist=s.astype(np.float32), dist64=s)
    return out


OUTPUTS = ("plane", "count", "best", "inlier", "dist")


def plane_numpy_batch(clouds, thresholds, H, seed, refine, axis=None, min_cos=0.0):
    """A ragged batch: (plane (S,4), count (S) int32, best (S) int32, inlier (total) uint8, dist (total) fp32)."""
    out = [plane_numpy(P, t, H, seed, refine, axis, min_cos) for P, t in zip(clouds, thresholds)]
    return (np.stack([o["plane"] for o in out]), np.asarray([o["count"] for o in out], np.int32),
            np.asarray([o["best"] for o in out], np.int32), np.concatenate([o["inlier"] for o in out]),
            np.concatenate([o["dist"] for o in out]))


def one(want):
    """The result of plane_numpy in the shape of a batch of one."""
    return (want["plane"][None], np.asarray([want["count"]], np.int32), np.asarray([want["best"]], np.int32),
            want["inlier"], want["dist"])


def equal(got, want):
    return all(same(np.asarray(g), np.asarray(w, np.asarray(g).dtype)) for g, w in zip(got, want))


# ---------------------------------------------------------------------------------------------
# the clouds (shared with tests/test_plane_gpu.py)
# ---------------------------------------------------------------------------------------------
def plane_and_sphere(n, seed=None):
    """Two thirds on the plane z = 0.3 x - 0.2 y + 0.1 with noise 0.005, the rest on a sphere above it; shuffled."""
    rng = np.random.RandomState(1000 + n if seed is None else seed)
    m = (2 * n) // 3
    xy = rng.uniform(-1, 1, (m, 2))
    flat = np.concatenate([xy, 0.3 * xy[:, :1] - 0.2 * xy[:, 1:] + 0.1 + 0.005 * rng.normal(size=(m, 1))], 1)
    ball = rng.normal(size=(n - m, 3))
    ball = 0.5 * ball / np.maximum(np.linalg.norm(ball, axis=1, keepdims=True), 1e-9) + np.asarray([0.0, 0.0, 1.0])
    P = np.concatenate([flat, ball]).astype(np.float32)
    return P[rng.permutation(n)]


def parallel_planes(n, seed=21):
    """55 % of the points on z = 0, 45 % on z = 0.5, both with noise 0.003."""
    rng = np.random.RandomState(seed)
    P = rng.uniform(-1, 1, (n, 3))
    m = (55 * n) // 100
    P[:, 2] = 0.003 * rng.normal(size=n) + np.where(np.arange(n) < m, 0.0, 0.5)
    return P.astype(np.float32)[rng.permutation(n)]


def perpendicular_planes(n, seed=22, share=0.6):
    """``share`` of the points on z = 0, the rest on x = 1.5 (beside it), noise 0.003: (cloud, on_floor bool)."""
    rng = np.random.RandomState(seed)
    P = rng.uniform(-1, 1, (n, 3))
    m = int(share * n)
    P[:m, 2] = 0.003 * rng.normal(size=m)
    P[m:, 0] = 1.5 + 0.003 * rng.normal(size=n - m)
    order = rng.permutation(n)
    return P.astype(np.float32)[order], (np.arange(n) < m)[order]


def lattice_plane(m):
    """The m x m lattice k / 8 on the plane z = 1: every valid hypothesis is (0, 0, 1, -1) exactly and holds all."""
    g = np.stack(np.meshgrid(np.arange(m), np.arange(m), indexing="ij"), -1).reshape(-1, 2) / 8.0
    return np.concatenate([g, np.ones((m * m, 1))], 1).astype(np.float32)


def at_the_threshold():
    """200 lattice points on z = 0, 100 at z = -0.125, 50 at z = 0.25 exactly and 50 one fp32 ulp above 0.25: with
    t = 0.25 and the axis (0, 0, 1) at max_angle 0 only horizontal planes are valid, and z = 0 holds the most: 350."""
    g = np.stack(np.meshgrid(np.arange(20), np.arange(20), indexing="ij"), -1).reshape(-1, 2) / 8.0
    z = np.concatenate([np.zeros(200), np.full(100, -0.125), np.full(50, 0.25),
                        np.full(50, np.nextafter(np.float32(0.25), np.float32(1)), np.float32)]).astype(np.float32)
    return np.concatenate([g.astype(np.float32), z[:, None]], 1)[np.random.RandomState(23).permutation(400)]


def exactly_collinear(n):
    """(1, 2, 3) + k (1/8, 1/4, -1/8): every coordinate and every difference is exact, every cross product 0."""
    k = np.arange(n, dtype=np.float64)[:, None]
    return (np.asarray([[1.0, 2.0, 3.0]]) + k * np.asarray([[0.125, 0.25, -0.125]])).astype(np.float32)


def triangle():
    return np.asarray([[0, 0, 0], [1, 0, 0.5], [0, 1, -0.25]], np.float32)


TABLETOP = dict(t=0.01, radius=0.25, seed=61)


def tabletop_scene():
    """(cloud (6000,3), part (6000)): 3 600 points of a table z = 0 with a z-jitter uniform in [-t/2, t/2] (part 0) and
    two tori of 1 200 points (parts 1 and 2; R = 1, r = 0.3, four apart) whose lowest points float 4.5 t above it."""
    from tests.test_cluster_abi import torus
    rng = np.random.RandomState(TABLETOP["seed"])
    t = TABLETOP["t"]
    table = np.stack([rng.uniform(-1.5, 5.5, 3600), rng.uniform(-1.5, 1.5, 3600), rng.uniform(-t / 2, t / 2, 3600)], 1)
    parts = [table.astype(np.float32)] + [torus(1200, TABLETOP["seed"] + 1 + k, centre=(4.0 * k, 0.0, 0.3 + 4.5 * t))
                                          for k in range(2)]
    order = rng.permutation(6000)
    return np.concatenate(parts)[order], np.repeat([0, 1, 2], [3600, 1200, 1200])[order]


UP, SIDE = (0.0, 0.0, 2.0), (1.0, 0.0, 0.0)      # (UP is not of unit length: the host normalises)
SIZES = (0, 1, 2, 3, 4, 63, 64, 65, 1023, 1024, 1025, 2049)
HS = (1, 2, 63, 64, 65, 100)
SEEDS = (3, 0xDEADBEEFCAFEF00D)


def case(cloud, t, H=64, seed=1, refine=1, axis=None, max_angle=None):
    return dict(cloud=cloud, t=t, H=H, seed=seed, refine=refine, axis=None if axis is None else unit_axis(axis),
                min_cos=0.0 if axis is None else min_cos_of(max_angle))


def cases():
    """name -> the arguments of one cloud."""
    out = {}
    for n in SIZES:
        out["plane and sphere %d" % n] = case(plane_and_sphere(n), 0.02)
    for H in HS:
        out["plane and sphere 1025, H %d" % H] = case(plane_and_sphere(1025), 0.02, H=H, seed=2)
    out["plane and sphere 1025, H 4096"] = case(plane_and_sphere(1025), 0.02, H=4096, seed=2, refine=4)
    out["plane and sphere 65, H 4096"] = case(plane_and_sphere(65), 0.02, H=4096, seed=2)
    for refine in (0, 1, 4):
        for seed in SEEDS:
            out["refine %d seed %x" % (refine, seed)] = case(plane_and_sphere(2049), 0.01, 100, seed, refine)
            out["refine %d seed %x axis" % (refine, seed)] = case(plane_and_sphere(2049), 0.01, 100, seed, refine, UP, 30)
    out["parallel planes"] = case(parallel_planes(1500), 0.01, H=100)
    out["parallel planes, refine 4"] = case(parallel_planes(1500), 0.004, H=100, refine=4)
    out["lattice plane"] = case(lattice_plane(20), 0.25, H=64, refine=1)
    out["at the threshold"] = case(at_the_threshold(), 0.25, H=64, refine=0, axis=UP, max_angle=0)
    out["collinear"] = case(exactly_collinear(300), 0.1, H=100)
    out["triangle, H 64"] = case(triangle(), 0.1, H=64)
    out["coincident"] = case(identical(50), 0.1, H=100)
    out["perpendicular planes"] = case(perpendicular_planes(1200)[0], 0.01, H=100)
    out["perpendicular planes, axis excludes the floor"] = case(perpendicular_planes(1200)[0], 0.01, 100, 1, 1, SIDE, 10)
    out["planar, axis excludes everything"] = case(planar(500), 0.01, 100, 1, 1, SIDE, 10)
    out["knn3: planar"] = case(planar(500), 0.01, H=100)
    out["knn3: collinear, refine 4"] = case(collinear(300), 0.02, H=65, refine=4)
    out["knn3: lattice"] = case(lattice(6), 0.01, H=100)
    out["knn3: offset cloud"] = case(offset_cloud(700), 1e-4, H=100, refine=4)
    out["knn3: copies among random"] = case(copies_among_random(600, 400), 0.05, H=100)
    return out


# the names of ``cases()``, literally: a case cannot go missing without a test that says so
CASES = (
    "at the threshold", "coincident", "collinear", "knn3: collinear, refine 4", "knn3: copies among random",
    "knn3: lattice", "knn3: offset cloud", "knn3: planar", "lattice plane", "parallel planes",
    "parallel planes, refine 4", "perpendicular planes", "perpendicular planes, axis excludes the floor",
    "planar, axis excludes everything", "plane and sphere 0", "plane and sphere 1", "plane and sphere 1023",
    "plane and sphere 1024", "plane and sphere 1025", "plane and sphere 1025, H 1", "plane and sphere 1025, H 100",
    "plane and sphere 1025, H 2", "plane and sphere 1025, H 4096", "plane and sphere 1025, H 63",
    "plane and sphere 1025, H 64", "plane and sphere 1025, H 65", "plane and sphere 2", "plane and sphere 2049",
    "plane and sphere 3", "plane and sphere 4", "plane and sphere 63", "plane and sphere 64", "plane and sphere 65",
    "plane and sphere 65, H 4096", "refine 0 seed 3", "refine 0 seed 3 axis", "refine 0 seed deadbeefcafef00d",
    "refine 0 seed deadbeefcafef00d axis", "refine 1 seed 3", "refine 1 seed 3 axis",
    "refine 1 seed deadbeefcafef00d", "refine 1 seed deadbeefcafef00d axis", "refine 4 seed 3",
    "refine 4 seed 3 axis", "refine 4 seed deadbeefcafef00d", "refine 4 seed deadbeefcafef00d axis", "triangle, H 64",
)


def test_the_case_list_is_literal():
    assert list(CASES) == sorted(cases())


BAD_THRESHOLDS = (0.0, -1.0, float("inf"), float("nan"))


def ragged_batches():
    """name -> (clouds, thresholds, H, seed, refine, axis, min_cos): empty segments first, in the middle and last; a NaN
    and an inf cloud among clean ones; thresholds that are none."""
    empty = np.zeros((0, 3), np.float32)
    nan, inf = plane_and_sphere(300, 5), plane_and_sphere(1031, 6)
    nan[11, 1], inf[1026, 0] = np.nan, -np.inf
    return {
        "empty first, middle and last": ([empty, plane_and_sphere(1300, 7), empty, empty, plane_and_sphere(70, 8),
                                          triangle(), empty], [0.02, 0.02, 0.02, 0.5, 0.01, 0.1, 0.02], 65, 9, 1, None, 0.0),
        "non-finite clouds among clean ones": ([plane_and_sphere(300, 5), nan, parallel_planes(1025), inf,
                                                plane_and_sphere(64, 4)], [0.02, 0.02, 0.01, 0.02, 0.03], 64, 10, 4,
                                               unit_axis(UP), min_cos_of(40)),
        "thresholds that are none": ([plane_and_sphere(65, 2), plane_and_sphere(65, 2), nan, plane_and_sphere(65, 2),
                                      plane_and_sphere(65, 2), empty, plane_and_sphere(65, 2)],
                                     [0.0, 0.02, float("nan"), -1.0, float("inf"), 0.0, float("nan")], 64, 11, 1, None,
                                     0.0),
    }


# ---------------------------------------------------------------------------------------------
# the host-compiled header
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    lib = native.build_harness(tmp_path_factory.mktemp("plh"), "plh", SOURCE)
    v, i, d, u = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_ulonglong
    lib.plh_plane.argtypes = [v, v, i, i, v, i, u, i, v, d, i, v, v, v, v, v]
    lib.plh_mix.restype, lib.plh_mix.argtypes = u, [u]
    lib.plh_draw.argtypes = [u, i, i, i]
    lib.plh_refit.argtypes = [v, v, i, v, d, v]
    return lib


def host_plane(lib, batch, thresholds, H, seed, refine, axis=None, min_cos=0.0, order=0):
    n = [c.shape[0] for c in batch]
    off = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
    S, total = len(batch), int(off[-1])
    P = np.ascontiguousarray(np.concatenate([c.reshape(-1, 3) for c in batch]), np.float32)
    t = np.asarray(thresholds, np.float32)
    plane, count, best = np.full((S, 4), -9.0), np.full(S, -9, np.int32), np.full(S, -9, np.int32)
    inlier, dist = np.full(total, 9, np.uint8), np.full(total, -9, np.float32)
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    ax = None if axis is None else np.ascontiguousarray(axis, np.float64)
    rc = lib.plh_plane(p(P), p(off), S, total, p(t), H, seed & M64, refine, p(ax), float(min_cos), order, p(plane),
                       p(count), p(best), p(inlier), p(dist))
    assert rc == 5 + 6 * refine
    return plane, count, best, inlier, dist


@pytest.fixture(scope="module")
def reference():
    """name -> plane_numpy of the case: computed once, shared, never changed."""
    return {name: plane_numpy(c["cloud"], c["t"], c["H"], c["seed"], c["refine"], c["axis"], c["min_cos"])
            for name, c in cases().items()}


def check_properties(c, want):
    """The exact properties of one result."""
    P, t64 = c["cloud"], np.float64(np.float32(c["t"]))
    assert int(want["inlier"].sum()) == max(want["count"], 0)
    assert same(want["dist"], want["dist64"].astype(np.float32))                # dist is the one rounding of the fp64 value
    if want["best"] < 0:
        assert want["count"] <= 0 and not want["plane"].any() and np.isnan(want["dist"]).all()
        return
    assert want["valid"][want["best"]] and want["count"] >= 1 and P.shape[0] >= 3
    assert np.array_equal(np.abs(want["dist64"]) <= t64, want["inlier"].astype(bool))
    nx, ny, nz, _ = (float(v) for v in want["plane"])
    norm2 = Fraction(nx) ** 2 + Fraction(ny) ** 2 + Fraction(nz) ** 2            # exact
    ulp = Fraction(1, 2 ** 52)
    assert (1 - ulp) ** 2 <= norm2 <= (1 + ulp) ** 2, float(norm2) - 1.0         # unit to 1 ulp
    lead = max((nx, ny, nz), key=abs)
    assert lead > 0 and same(np.asarray(canonical(nx, ny, nz), np.float64), want["plane"][:3])
    if c["axis"] is not None:
        assert abs(dot3(nx, ny, nz, *c["axis"])) >= c["min_cos"]


@pytest.mark.parametrize("name", CASES)
def test_the_simulated_schedule_equals_the_definition(harness, reference, name):
    c, want = cases()[name], reference[name]
    for order in (0, 1):
        got = host_plane(harness, [c["cloud"]], [c["t"]], c["H"], c["seed"], c["refine"], c["axis"], c["min_cos"], order)
        assert equal(got, one(want)), (name, order)
    check_properties(c, want)
    n = c["cloud"].shape[0]
    if name.startswith("plane and sphere") and n >= 63 and c["H"] >= 63:       # the plane is found
        assert want["best"] >= 0 and (2 * n) // 6 <= want["count"] <= (2 * n) // 3 + 0.05 * n + 2, want["count"]
    if name.startswith("plane and sphere") and n < 3:
        assert want["best"] == -1 and want["count"] == 0
    if name.startswith("refine"):
        assert want["best"] >= 0 and want["count"] > 0.5 * n
    if name == "parallel planes":
        assert abs(want["plane"][3]) < 0.01 and abs(want["count"] - (55 * n) // 100) <= 5    # the larger one
    if name == "lattice plane":
        assert want["count"] == n and want["best"] == int(np.flatnonzero(want["valid"])[0])   # the tie rule
        assert want["plane"].tolist() == [0.0, 0.0, 1.0, -1.0] and 0 < want["valid"].sum() < c["H"]
    if name == "at the threshold":
        z = c["cloud"][:, 2]
        assert want["plane"].tolist() == [0.0, 0.0, 1.0, 0.0] and want["count"] == 350
        assert want["inlier"][z == np.float32(0.25)].all() and not want["inlier"][z > np.float32(0.25)].any()
        assert (z > np.float32(0.25)).sum() == 50 and (want["dist"][z == np.float32(0.25)] == np.float32(0.25)).all()
    if name == "collinear" or name == "coincident" or name == "planar, axis excludes everything":
        assert want["best"] == -1 and want["count"] == 0 and not want["valid"].any()
    if name == "triangle, H 64":
        assert 0 < want["valid"].sum() < 64 and want["count"] == 3
    if name == "perpendicular planes":
        assert abs(want["plane"][2]) > 0.99 and want["count"] >= 700
    if name == "perpendicular planes, axis excludes the floor":
        assert abs(want["plane"][0]) > 0.99 and 400 <= want["count"] <= 500    # the second plane wins
    if name == "knn3: planar":
        assert want["count"] == n


def test_the_hash_and_the_draws(harness):
    assert harness.plh_mix(0) == mix(0) == 0
    for z in (1, GOLD, M64, 0x0123456789ABCDEF):
        assert harness.plh_mix(z) == mix(z), z
    assert mix(GOLD) == 0xE220A8397B1DCDAF                     # the first output of splitmix64 seeded with 0
    for seed in SEEDS + (0, M64):
        for n in (1, 3, 1025, 2 ** 31 - 1):
            idx = draws(seed, 8, n)
            assert idx.min() >= 0 and idx.max() < n
            assert idx.tolist() == [[harness.plh_draw(seed, h, s, n) for s in range(3)] for h in range(8)]


def test_the_constants_are_the_ones_the_tests_assume(harness):
    assert [harness.plh_constant(k) for k in range(5)] == [1024, 4096, 4, SWEEPS, 6]
    assert [harness.plh_launches(r) for r in (-1, 0, 1, 4, 5)] == [0, 5, 11, 29, 0]


@pytest.mark.parametrize("name", sorted(ragged_batches()))
def test_a_cloud_gives_the_same_bits_alone_and_at_any_position_of_a_batch(harness, name):
    clouds, ts, H, seed, refine, axis, min_cos = ragged_batches()[name]
    want = plane_numpy_batch(clouds, ts, H, seed, refine, axis, min_cos)
    for order in (0, 1):
        assert equal(host_plane(harness, clouds, ts, H, seed, refine, axis, min_cos, order), want), (name, order)
    o = 0
    for c, P in enumerate(clouds):                                           # every cloud alone gives what it gives here
        alone = host_plane(harness, [P], [ts[c]], H, seed, refine, axis, min_cos)
        n = P.shape[0]
        assert equal(alone, (want[0][c:c + 1], want[1][c:c + 1], want[2][c:c + 1], want[3][o:o + n], want[4][o:o + n]))
        o += n
    back = host_plane(harness, clouds[::-1], ts[::-1], H, seed, refine, axis, min_cos)
    assert equal(back[:3], [w[::-1] for w in want[:3]])
    if name == "empty first, middle and last":
        assert want[1].tolist()[0] == 0 and want[2].tolist()[0] == -1 and want[1][1] > 800 and want[1][5] == 3
    if name == "non-finite clouds among clean ones":
        assert want[1].tolist()[1] == -1 and want[1][3] == -1 and (want[1][[0, 2, 4]] > 30).all()
        assert not want[3][300:600].any() and np.isnan(want[4][300:600]).all()
    if name == "thresholds that are none":
        assert want[1].tolist() == [-2, want[1][1], -1, -2, -2, -2, -2] and want[1][1] > 30
        assert (want[2][[0, 2, 3, 4, 5, 6]] == -1).all()
        assert [threshold_status(t) for t in BAD_THRESHOLDS] == [-2] * 4


def test_the_tabletop_scene_by_the_definition():
    """The scene of tests/test_plane_gpu.py on the CPU, before a GPU ever runs: with the default seed and the scene's
    generator seed the restatement alone finds the table exactly, the clusters see one object with it and the two tori
    without it."""
    from tests.test_cluster_abi import cluster_numpy
    P, part = tabletop_scene()
    t, r = TABLETOP["t"], TABLETOP["radius"]
    assert (np.abs(P[part == 0][:, 2]) <= np.float32(t / 2)).all() and P[part != 0][:, 2].min() >= 4 * t
    want = plane_numpy(P, t, 512, 0, 1, unit_axis((0, 0, 1)), min_cos_of(10))
    assert want["best"] >= 0 and same(want["inlier"], (part == 0).astype(np.uint8)) and want["count"] == 3600
    assert cluster_numpy(P, r)[1] == 1
    label, C = cluster_numpy(P[part != 0], r)[:2]
    assert C == 2 and all(len(set(part[part != 0][label == k])) == 1 for k in range(2))


def test_refinement_never_loses_inliers(harness):
    for P, t, axis, min_cos in ((plane_and_sphere(2049), 0.01, None, 0.0), (parallel_planes(1500), 0.004, None, 0.0),
                                (perpendicular_planes(1200)[0], 0.005, unit_axis(UP), min_cos_of(20)),
                                (offset_cloud(700), 1e-4, None, 0.0), (lattice(6), 0.3, None, 0.0)):
        for seed in SEEDS:
            before, best = -1, None
            for refine in range(5):
                plane, count, b, inlier, _ = host_plane(harness, [P], [t], 32, seed, refine, axis, min_cos)
                assert b[0] >= 0 and count[0] >= before and inlier.sum() == count[0]
                assert best in (None, b[0])                                  # best does not depend on the refinement
                before, best = count[0], b[0]


def test_the_jacobi_agrees_with_numpy_eigh(harness):
    """The solver of the refit against numpy.linalg.eigh under the bar of tests/test_point_normals_abi.py for the same
    solver: BAR = 4 E radians wherever the reference's gap (l1 - l0) / l2 is at least GAP_MIN."""
    rng = np.random.RandomState(31)
    checked = 0
    for trial in range(200):
        R = np.linalg.qr(rng.normal(size=(3, 3)))[0]
        X = (rng.normal(size=(300, 3)) * np.asarray([1.0, rng.uniform(0.05, 1.0), rng.uniform(0.0, 0.05)])) @ R.T
        X = X + rng.uniform(-5, 5, (1, 3))
        mean = X.mean(0)
        D = X - mean
        C = D.T @ D
        sums = np.asarray([C[0, 0], C[0, 1], C[0, 2], C[1, 1], C[1, 2], C[2, 2]])
        out = np.zeros(4)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
        ok = harness.plh_refit(p(mean), p(sums), 300, None, 0.0, p(out))
        mine = refit_python(mean, sums, 300, None, 0.0)
        assert ok == 1 and mine is not None and same(out, np.asarray(mine, np.float64))      # the two restatements
        w, v = np.linalg.eigh(C / 300.0)
        if (w[1] - w[0]) / w[2] < GAP_MIN:
            continue
        checked += 1
        cos = abs(float(np.dot(v[:, 0], out[:3])))
        cross = np.linalg.norm(np.cross(v[:, 0], out[:3]))
        assert math.atan2(cross, cos) <= BAR, (trial, math.atan2(cross, cos))
        assert abs(out[3] + np.dot(out[:3], mean)) <= 1e-12 * (1 + np.abs(mean).max())
    assert checked >= 150
    assert refit_python([0, 0, 0], [0.0] * 6, 10, None, 0.0) is None          # coincident: degenerate
    assert refit_python([0, 0, 0], [1.0, 0, 0, 1.0, 0, 0], 2, None, 0.0) is None          # fewer than three points


def test_the_program_under_the_sanitizers_over_the_case_list(tmp_path, reference):
    """The same file with its main, built with -fsanitize=address,undefined (the runtimes linked into the program) and
    run once over its own list (both orders of arrival against a brute force) and once over every case of ``cases()``
    from a file, in both orders.  It runs in the environment it finds: nothing is preloaded or set for it."""
    exe = os.path.join(str(tmp_path), "plane_host")
    subprocess.run(native.GXX + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                 "-static-libasan", "-static-libubsan", "-o", exe, SOURCE], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and " 0 differences" in run.stdout and run.stderr == "", (run.stdout, run.stderr)
    names = sorted(cases())
    path = tmp_path / "clouds.txt"
    with open(path, "w") as f:
        for name in names:
            c = cases()[name]
            ax = [0.0, 0.0, 0.0] if c["axis"] is None else c["axis"].tolist()
            f.write("%d %.9g %d %d %d %d %.17g %.17g %.17g %.17g\n" % (c["cloud"].shape[0], np.float32(c["t"]), c["H"],
                                                                      c["seed"], c["refine"], c["axis"] is not None,
                                                                      ax[0], ax[1], ax[2], c["min_cos"]))
            f.write("".join("%.9g %.9g %.9g\n" % tuple(p) for p in c["cloud"].tolist()))
    run = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-2000:]
    words = iter(run.stdout.split())
    for name in names:
        want = reference[name]
        assert [int(next(words)), int(next(words))] == [want["count"], want["best"]], name
        assert same(np.asarray([float(next(words)) for _ in range(4)]), want["plane"]), name
        rows = [(int(next(words)), np.float32(next(words))) for _ in range(want["inlier"].shape[0])]
        assert same(np.asarray([r[0] for r in rows], np.uint8).reshape(-1), want["inlier"]), name
        assert same(np.asarray([r[1] for r in rows], np.float32).reshape(-1), want["dist"]), name
    assert next(words, None) is None


# ---------------------------------------------------------------------------------------------
# the exports, the schedule, the workspace and the argument checks, which run before anything touches a GPU
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    return native.load_raw(NAMES)


def test_the_entry_points_are_exported_and_bound(lib, harness):
    from parsenet_codebase_amd import _lib
    v, i, ll, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_double
    assert _lib.SIGNATURES["pn_plane_f32"] == (i, [v, v, i, i, v, i, ll, i, v, d, v, v, v, v, v, v, ll, v])
    assert _lib.SIGNATURES["pn_plane_workspace_bytes"] == (ll, [ll, i, i])
    assert _lib.SIGNATURES["pn_plane_launches"] == (i, [i])
    assert lib.pn_abi_version() == 23 == _lib.CONSTANTS["PN_ABI_VERSION"]                   # added symbols only
    assert all(hasattr(_lib.load(), n) for n in NAMES)
    for refine, want in ((0, 5), (1, 11), (2, 17), (3, 23), (4, 29), (-1, 0), (5, 0)):       # 5 + 6 refine
        assert lib.pn_plane_launches(refine) == harness.plh_launches(refine) == want, refine
    w = lib.pn_plane_workspace_bytes
    for total, S, H in ((1, 1, 1), (1024, 3, 512), (10 ** 6, 7, 4096), (2 ** 31 - 1, 1, 64), (0, 5, 100),
                        (40000, 4, 512)):
        assert w(total, S, H) == 36 * S * H + 64 * (total // 1024 + S) + 60 * S + 16, (total, S, H)   # the header's
    assert w(2 ** 31, 1, 64) == 0 and w(-1, 1, 64) == 0 and w(10, -1, 64) == 0
    assert w(10, 1, 0) == 0 and w(10, 1, 4097) == 0 and w(10, 1, -3) == 0


ARGS = ("pts", "off", "S", "total", "threshold", "H", "seed", "refine", "axis", "min_cos", "plane", "count", "best",
        "inlier", "dist", "ws", "ws_bytes", "stream")


def raw_call(lib, **over):
    """pn_plane_f32 with plausible arguments (never dereferenced by a call that is refused), some replaced."""
    a = dict(pts=64, off=64, S=1, total=10, threshold=64, H=64, seed=-1, refine=1, axis=None, min_cos=0.0, plane=64,
             count=64, best=64, inlier=64, dist=None, ws=64, ws_bytes=lib.pn_plane_workspace_bytes(10, 1, 64),
             stream=None)
    a.update(over)
    return lib.pn_plane_f32(*[a[n] for n in ARGS])


def test_invalid_arguments_are_refused_before_any_launch(lib):
    """(No GPU is needed to get here: a refused call, and one with nothing to do, launch nothing.)"""
    from parsenet_codebase_amd import _lib
    err = _lib.CONSTANTS["PN_ERR_ARG"]
    need = lib.pn_plane_workspace_bytes(10, 1, 64)
    for over, word in ((dict(S=-1), b"S=-1"), (dict(total=-1), b"total=-1"), (dict(H=0), b"H=0"),
                       (dict(H=4097, ws_bytes=1 << 30), b"H=4097"), (dict(H=-1), b"H=-1"),
                       (dict(refine=-1), b"refine=-1"), (dict(refine=5), b"refine=5"),
                       (dict(axis=64, min_cos=1.5), b"min_cos=1.5"), (dict(axis=64, min_cos=-0.1), b"min_cos=-0.1"),
                       (dict(axis=64, min_cos=float("nan")), b"min_cos="),
                       (dict(S=2 ** 20, H=4096, ws_bytes=1 << 62), b"S * H"),
                       (dict(pts=None), b"null"), (dict(off=None), b"null"), (dict(threshold=None), b"null"),
                       (dict(plane=None), b"null"), (dict(count=None), b"null"), (dict(best=None), b"null"),
                       (dict(inlier=None), b"null"), (dict(ws=None), b"null"),
                       (dict(ws_bytes=need - 1), b"workspace"), (dict(ws_bytes=0), b"workspace")):
        assert raw_call(lib, **over) == err, over
        assert b"pn_plane_f32" in lib.pn_last_error() and word in lib.pn_last_error(), (over, lib.pn_last_error())
    assert raw_call(lib, S=0) == 0 and raw_call(lib, total=0) == 0
    assert raw_call(lib, S=0, pts=None, plane=None, count=None, inlier=None, ws=None, ws_bytes=0) == 0
    assert raw_call(lib, total=0, pts=None, threshold=None, ws=None, ws_bytes=0) == 0
    assert raw_call(lib, S=0, H=0) == err and raw_call(lib, total=0, refine=9) == err      # the arguments come first
    assert raw_call(lib, S=0, min_cos=7.0) == 0                                            # (no axis: min_cos is not read)


def test_python_argument_checks_need_no_gpu():
    import torch
    from parsenet_codebase_amd import cleaning, kernels
    P = torch.zeros(8, 3)
    off = torch.tensor([0, 8], dtype=torch.int32)
    with pytest.raises(TypeError, match="must be on the GPU"):
        kernels.plane_ragged(P, off, torch.ones(1))
    with pytest.raises(TypeError, match="plane_ragged: threshold must be a tensor"):
        kernels.plane_ragged(P, off, 0.1)
    for H in (0, 4097, 1.5, True, None, "64"):
        with pytest.raises(ValueError, match="plane_ragged: hypotheses must be"):
            kernels.plane_ragged(P, off, torch.ones(1), hypotheses=H)
    for refine in (-1, 5, 1.0, True, None):
        with pytest.raises(ValueError, match="plane_ragged: refine must be"):
            kernels.plane_ragged(P, off, torch.ones(1), refine=refine)
    for seed in (1.5, True, None, 2 ** 64, -2 ** 63 - 1):
        with pytest.raises(ValueError, match="plane_ragged: seed must be"):
            kernels.plane_ragged(P, off, torch.ones(1), seed=seed)
    for axis, angle in (((0, 0, 1), None), (None, 10)):
        with pytest.raises(ValueError, match="axis and max_angle come together"):
            kernels.plane_ragged(P, off, torch.ones(1), axis=axis, max_angle=angle)
    for axis in ((0, 0, 0), (0, float("nan"), 1), (float("inf"), 0, 0), (1, 2), "abc", (1e200, 1e200, 1e200)):
        with pytest.raises(ValueError, match="plane_ragged: axis must be"):
            kernels.plane_ragged(P, off, torch.ones(1), axis=axis, max_angle=10)
    for angle in (91, -1, float("nan"), True, "10"):
        with pytest.raises(ValueError, match="plane_ragged: max_angle must be"):
            kernels.plane_ragged(P, off, torch.ones(1), axis=(0, 0, 1), max_angle=angle)
    with pytest.raises(ValueError, match="plane_ragged: want holds"):
        kernels.plane_ragged(P, off, torch.ones(1), want=("count",))
    for fn in (cleaning.fit_plane, cleaning.remove_plane):
        for t in (0, -1, float("inf"), float("nan"), True, "a", 1e-60, [0.0], None):
            with pytest.raises(ValueError, match="threshold must be"):
                fn(P, threshold=t)
        with pytest.raises(ValueError, match="threshold holds one number per cloud"):
            fn([P, P], threshold=[0.1, 0.2, 0.3])
        with pytest.raises(RuntimeError, match="MI355X only"):
            fn(P, threshold=0.1)
    with pytest.raises(ValueError, match='keep must be "rest" or "plane"'):
        cleaning.remove_plane(P, threshold=0.1, keep="both")
    for over in (dict(max_planes=0), dict(min_inliers=0), dict(max_planes=True), dict(min_inliers=1.5), dict(seed=0.5)):
        with pytest.raises(ValueError, match="peel_planes: "):
            cleaning.peel_planes(P, **dict(dict(threshold=0.1, max_planes=2, min_inliers=10), **over))
    with pytest.raises(ValueError, match="peel_planes: one cloud"):
        cleaning.peel_planes([P], threshold=0.1, max_planes=2, min_inliers=10)
    assert np.array_equal(kernels._plane_axis("t", UP, 30)[0], unit_axis(UP))
    assert kernels._plane_axis("t", UP, 30)[1] == min_cos_of(30) and kernels._plane_axis("t", UP, 90)[1] >= 0.0
