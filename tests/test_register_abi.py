"""CPU-side checks of the rigid registration: csrc/register_math.h compiled for the host into a serial simulation of the
kernels' schedule (tests/native/register_host.cpp: the target's grid, then per iteration move, pair, the two passes of
sums over the tree of csrc/outlier_math.h, the solve and the stopping rule, then the final evaluation) against
``register_numpy``, an independent numpy / Python restatement written from the definition (brute-force nearest neighbours
under the fp32 key (d, j), the tree sums of tests/test_outlier_abi.py, quaternions, the 4 x 4 Jacobi and the 6 x 6 LDL^T in
Python floats) — every output equal bit for bit, with both orders of the tiles —, the properties of the definition on
scans, the stand-alone program under the address and undefined-behaviour sanitizers, and the exports of csrc/register.hip,
their schedule and argument checks."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from tests.helpers import native
from tests.test_fps_abi import same
from tests.test_outlier_abi import tree_sum

SOURCE = native.source("register_host.cpp")
NAMES = ("pn_register_f32", "pn_register_launches", "pn_register_workspace_bytes", "pn_rigid_apply_f32")
POINT, PLANE = 0, 1
CONVERGED, MAX_ITER, TOO_FEW, DEGENERATE, NON_FINITE = 0, 1, 2, 3, 4
SWEEPS = 5           # RR_SWEEPS of csrc/register_math.h   (test_the_constants_are_the_ones_the_tests_assume)
PIVOT = 1e-12        # RR_PIVOT
INF = float("inf")


# ---------------------------------------------------------------------------------------------
# the definition, in numpy and Python (shared with tests/test_register_gpu.py)
# ---------------------------------------------------------------------------------------------
def rotation_of(q):
    w, x, y, z = q
    xx, yy, zz, xy, xz, yz, wx, wy, wz = x * x, y * y, z * z, x * y, x * z, y * z, w * x, w * y, w * z
    return [[1.0 - 2.0 * (yy + zz), 2.0 * (xy - wz), 2.0 * (xz + wy)],
            [2.0 * (xy + wz), 1.0 - 2.0 * (xx + zz), 2.0 * (yz - wx)],
            [2.0 * (xz - wy), 2.0 * (yz + wx), 1.0 - 2.0 * (xx + yy)]]


def normalised(q):
    n = math.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    return [q[0] / n, q[1] / n, q[2] / n, q[3] / n]


def first_positive(q):
    lead = next((c for c in q if c != 0.0), 0.0)
    return [-c for c in q] if lead < 0.0 else list(q)


def state_of(M):
    """(q, t) of a 4 x 4 by the extraction rule."""
    M = [[float(v) for v in row] for row in np.asarray(M, np.float64).reshape(4, 4)]
    tr = (M[0][0] + M[1][1]) + M[2][2]
    k, best = 0, tr
    for c, v in ((1, M[0][0]), (2, M[1][1]), (3, M[2][2])):
        if v > best:
            k, best = c, v
    if k == 0:
        q = [1.0 + tr, M[2][1] - M[1][2], M[0][2] - M[2][0], M[1][0] - M[0][1]]
    elif k == 1:
        q = [M[2][1] - M[1][2], ((1.0 + M[0][0]) - M[1][1]) - M[2][2], M[0][1] + M[1][0], M[0][2] + M[2][0]]
    elif k == 2:
        q = [M[0][2] - M[2][0], M[0][1] + M[1][0], ((1.0 - M[0][0]) + M[1][1]) - M[2][2], M[1][2] + M[2][1]]
    else:
        q = [M[1][0] - M[0][1], M[0][2] + M[2][0], M[1][2] + M[2][1], ((1.0 - M[0][0]) - M[1][1]) + M[2][2]]
    return first_positive(normalised(q)), [M[0][3], M[1][3], M[2][3]]


def matrix_of(q, t):
    R = rotation_of(q)
    return np.asarray([R[0] + [t[0]], R[1] + [t[1]], R[2] + [t[2]], [0.0, 0.0, 0.0, 1.0]], np.float64)


def move_numpy(P, q, t):
    """The move step on (n,3) fp32 -> (n,3) fp32."""
    R = rotation_of(q)
    X = np.asarray(P, np.float32).reshape(-1, 3).astype(np.float64)
    with np.errstate(all="ignore"):
        return np.stack([((R[a][0] * X[:, 0] + R[a][1] * X[:, 1]) + R[a][2] * X[:, 2]) + t[a] for a in range(3)],
                        1).astype(np.float32)


def apply_numpy(P, M):
    return move_numpy(P, *state_of(M))


def nearest_numpy(Q, T):
    """idx (n) int32 and dist (n) fp32 of the k = 1 cross-cloud query by brute force under the key (d, j)."""
    Q, T = np.asarray(Q, np.float32).reshape(-1, 3), np.asarray(T, np.float32).reshape(-1, 3)
    n = Q.shape[0]
    idx, dist = np.full(n, -1, np.int32), np.full(n, np.nan, np.float32)
    if not np.isfinite(T).all():
        return idx, dist
    ok = np.isfinite(Q).all(1)
    if T.shape[0] == 0:
        dist[ok] = np.inf
        return idx, dist
    rows = np.flatnonzero(ok)
    for c in range(0, rows.shape[0], 1024):
        r = rows[c:c + 1024]
        dx, dy, dz = (Q[r, None, a] - T[None, :, a] for a in range(3))
        with np.errstate(over="ignore"):
            d = (dx * dx + dy * dy) + dz * dz
        j = d.argmin(1)                                                        # the first of equal minima
        idx[r] = j
        dist[r] = np.sqrt(d[np.arange(r.shape[0]), j].astype(np.float64)).astype(np.float32)
    return idx, dist


def qmul(a, b):
    return [((a[0] * b[0] - a[1] * b[1]) - a[2] * b[2]) - a[3] * b[3],
            ((a[0] * b[1] + a[1] * b[0]) + a[2] * b[3]) - a[3] * b[2],
            ((a[0] * b[2] - a[1] * b[3]) + a[2] * b[0]) + a[3] * b[1],
            ((a[0] * b[3] + a[1] * b[2]) - a[2] * b[1]) + a[3] * b[0]]


def rotate(R, v):
    return [(R[a][0] * v[0] + R[a][1] * v[1]) + R[a][2] * v[2] for a in range(3)]


def horn_python(S, sweeps=SWEEPS):
    """dq of the nine sums S[a][b]: Horn's matrix and the cyclic Jacobi in Python floats."""
    (sxx, sxy, sxz), (syx, syy, syz), (szx, szy, szz) = S
    A = [[0.0] * 4 for _ in range(4)]
    A[0][0], A[0][1], A[0][2], A[0][3] = (sxx + syy) + szz, syz - szy, szx - sxz, sxy - syx
    A[1][1], A[1][2], A[1][3] = (sxx - syy) - szz, sxy + syx, szx + sxz
    A[2][2], A[2][3] = (syy - sxx) - szz, syz + szy
    A[3][3] = (szz - sxx) - syy
    for i in range(4):
        for j in range(i):
            A[i][j] = A[j][i]
    V = [[1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
    for _ in range(sweeps):
        for p in range(3):
            for q in range(p + 1, 4):
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
                for k in range(4):
                    if k != p and k != q:
                        akp, akq = A[k][p], A[k][q]
                        A[k][p] = A[p][k] = c * akp - s * akq
                        A[k][q] = A[q][k] = s * akp + c * akq
                    vp, vq = V[k][p], V[k][q]
                    V[k][p] = c * vp - s * vq
                    V[k][q] = s * vp + c * vq
    col = 0
    for k in range(1, 4):
        if A[k][k] > A[col][col]:
            col = k
    return first_positive(normalised([V[k][col] for k in range(4)]))


def ldlt_python(sums):
    """x (6) of A x = -b from the 21 + 6 sums, or None when a pivot is not above PIVOT times the largest diagonal."""
    A = [[0.0] * 6 for _ in range(6)]
    e = 0
    for i in range(6):
        for j in range(i, 6):
            A[i][j] = A[j][i] = float(sums[e])
            e += 1
    floor = PIVOT * max(A[j][j] for j in range(6))
    L = [[0.0] * 6 for _ in range(6)]
    d = [0.0] * 6
    for j in range(6):
        dj = A[j][j]
        for k in range(j):
            dj = dj - (L[j][k] * L[j][k]) * d[k]
        if not dj > floor:
            return None
        d[j] = dj
        for i in range(j + 1, 6):
            v = A[i][j]
            for k in range(j):
                v = v - (L[i][k] * L[j][k]) * d[k]
            L[i][j] = v / dj
    y = [0.0] * 6
    for i in range(6):
        z = -float(sums[21 + i])
        for k in range(i):
            z = z - L[i][k] * y[k]
        y[i] = z
    y = [y[i] / d[i] for i in range(6)]
    x = [0.0] * 6
    for i in range(5, -1, -1):
        z = y[i]
        for k in range(i + 1, 6):
            z = z - L[k][i] * x[k]
        x[i] = z
    return x


def accepted_numpy(idx, dist, max_dist, normals):
    with np.errstate(invalid="ignore"):
        acc = (idx >= 0) & (dist <= np.float32(max_dist))
    if normals is not None and normals.shape[0]:
        acc &= np.isfinite(normals[np.maximum(idx, 0)]).all(1)
    return acc


def register_numpy(src, tgt, max_dist, mode=POINT, normals=None, max_iter=50, tol_rot=1e-6, tol_trans=1e-6, init=None,
                   sweeps=SWEEPS, trace=None):
    """One segment pair by the definition -> a dict: transform (4,4) fp64, iterations, status, count, rmse, idx (n) int32,
    dist (n) fp32.  ``trace``: a list that receives the nine sums of every point-mode iteration."""
    src = np.ascontiguousarray(src, np.float32).reshape(-1, 3)
    tgt = np.ascontiguousarray(tgt, np.float32).reshape(-1, 3)
    nrm = None if mode == POINT else np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    T64 = tgt.astype(np.float64)
    q, t = ([1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0]) if init is None else state_of(init)
    bad = not np.isfinite(tgt).all()
    status, iterations = MAX_ITER, 0
    for it in range(1, max_iter + 1):
        iterations = it
        P = move_numpy(src, q, t)
        idx, dist = nearest_numpy(P, tgt)
        acc = accepted_numpy(idx, dist, max_dist, nrm)
        m = int(acc.sum())
        if bad:
            status = NON_FINITE
            break
        if m < (6 if mode == PLANE else 3):
            status = TOO_FEW
            break
        j = np.maximum(idx, 0)
        P64, Q64 = P.astype(np.float64), T64[j]
        with np.errstate(all="ignore"):
            mean = [float(tree_sum(np.where(acc, P64[:, a], 0.0)) / np.float64(m)) for a in range(3)]
            mean += [float(tree_sum(np.where(acc, Q64[:, a], 0.0)) / np.float64(m)) for a in range(3)]
            c = [P64[:, a] - mean[a] for a in range(3)]
            if mode == POINT:
                b = [Q64[:, a] - mean[3 + a] for a in range(3)]
                S = [[float(tree_sum(np.where(acc, c[a] * b[e], 0.0))) for e in range(3)] for a in range(3)]
                if trace is not None:
                    trace.append(S)
                dq = horn_python(S, sweeps)
                dR = rotation_of(dq)
                rp = rotate(dR, mean[:3])
                dt = [mean[3 + a] - rp[a] for a in range(3)]
            else:
                n = [nrm[j][:, a].astype(np.float64) for a in range(3)]
                d = [P64[:, a] - Q64[:, a] for a in range(3)]
                r = (n[0] * d[0] + n[1] * d[1]) + n[2] * d[2]
                row = [c[1] * n[2] - c[2] * n[1], c[2] * n[0] - c[0] * n[2], c[0] * n[1] - c[1] * n[0], n[0], n[1], n[2]]
                sums = [tree_sum(np.where(acc, row[i] * row[k], 0.0)) for i in range(6) for k in range(i, 6)]
                sums += [tree_sum(np.where(acc, row[k] * r, 0.0)) for k in range(6)]
                x = ldlt_python(sums)
                if x is None:
                    status = DEGENERATE
                    break
                dq = normalised([1.0, x[0] / 2.0, x[1] / 2.0, x[2] / 2.0])
                dR = rotation_of(dq)
                rp = rotate(dR, mean[:3])
                dt = [(mean[a] + x[3 + a]) - rp[a] for a in range(3)]
            nq = normalised(qmul(dq, q))
            rt = rotate(dR, t)
            nt = [rt[a] + dt[a] for a in range(3)]
        if not all(math.isfinite(v) for v in nq + nt):
            status = DEGENERATE
            break
        q, t = nq, nt
        rot = 2.0 * math.sqrt((dq[1] * dq[1] + dq[2] * dq[2]) + dq[3] * dq[3])
        e = [(rp[a] + dt[a]) - mean[a] for a in range(3)]
        if rot <= tol_rot and math.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) <= tol_trans:
            status = CONVERGED
            break
    P = move_numpy(src, q, t)
    idx, dist = nearest_numpy(P, tgt)
    acc = accepted_numpy(idx, dist, max_dist, nrm)
    m = int(acc.sum())
    d64 = dist.astype(np.float64)
    with np.errstate(all="ignore"):
        res = tree_sum(np.where(acc, d64 * d64, 0.0))
        rmse = np.sqrt(res / np.float64(m)) if m else np.float64(np.nan)
    return dict(transform=matrix_of(q, t), iterations=iterations, status=status, count=m, rmse=float(rmse), idx=idx,
                dist=dist)


OUTPUTS = ("transform", "iterations", "status", "count", "rmse", "idx", "dist")


def register_numpy_batch(case):
    """A ragged batch: (transform (S,16), iterations, status, count (S) int32, rmse (S), idx (total), dist (total))."""
    S = len(case["src"])
    out = [register_numpy(case["src"][s], case["tgt"][s], case["max_dist"], case["mode"],
                          None if case["normals"] is None else case["normals"][s], case["max_iter"], case["tol"][0],
                          case["tol"][1], None if case["init"] is None else case["init"][s]) for s in range(S)]
    return batch_of(out)


def batch_of(out):
    return (np.stack([o["transform"].reshape(16) for o in out]).reshape(-1, 16),
            np.asarray([o["iterations"] for o in out], np.int32), np.asarray([o["status"] for o in out], np.int32),
            np.asarray([o["count"] for o in out], np.int32), np.asarray([o["rmse"] for o in out], np.float64),
            np.concatenate([o["idx"] for o in out] + [np.zeros(0, np.int32)]),
            np.concatenate([o["dist"] for o in out] + [np.zeros(0, np.float32)]))


def equal(got, want):
    return all(same(np.asarray(g), np.asarray(w, np.asarray(g).dtype).reshape(np.asarray(g).shape))
               for g, w in zip(got, want))


def which_differ(got, want):
    return [n for n, g, w in zip(OUTPUTS, got, want) if not equal([g], [w])]


# ---------------------------------------------------------------------------------------------
# the clouds (shared with tests/test_register_gpu.py)
# ---------------------------------------------------------------------------------------------
JITTER = 0.002


def scan(n, seed=5):
    """(cloud (n,3) fp32, normals (n,3) fp32): a torus (R = 1, r = 0.3) with a jitter of JITTER and, from a tenth of its
    points, a bump — a cap of radius 0.2 about (1.3, 0.1, 0.12) — that breaks every symmetry of the torus."""
    rng = np.random.RandomState(seed)
    u, v = rng.uniform(0, 2 * np.pi, n), rng.uniform(0, 2 * np.pi, n)
    nrm = np.stack([np.cos(v) * np.cos(u), np.cos(v) * np.sin(u), np.sin(v)], 1)
    P = np.stack([np.cos(u), np.sin(u), np.zeros(n)], 1) + 0.3 * nrm
    b = n // 10
    d = rng.normal(size=(b, 3))
    d[:, 0] = np.abs(d[:, 0])
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    P[:b], nrm[:b] = np.asarray([1.3, 0.1, 0.12]) + 0.2 * d, d
    P = P + JITTER * rng.uniform(-1, 1, (n, 3))
    order = rng.permutation(n)
    return P[order].astype(np.float32), nrm[order].astype(np.float32)


def motion(degrees, axis=(1.0, 2.0, 3.0), shift=(0.05, -0.03, 0.04)):
    """The 4 x 4 of a rotation by ``degrees`` about ``axis`` and a translation (Rodrigues in fp64)."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.asarray([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = math.radians(degrees)
    M = np.eye(4)
    M[:3, :3] = np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)
    M[:3, 3] = shift
    return M


def moved(P, M):
    return (P.astype(np.float64) @ M[:3, :3].T + M[:3, 3]).astype(np.float32)


def case(src, tgt, max_dist=INF, mode=POINT, normals=None, max_iter=8, tol=(1e-6, 1e-6), init=None):
    one = not isinstance(src, list)
    return dict(src=[src] if one else src, tgt=[tgt] if one else tgt, max_dist=max_dist, mode=mode,
                normals=None if mode == POINT else ([normals] if one else normals), max_iter=max_iter, tol=tol,
                init=None if init is None else ([init] if one else init))


EMPTY = np.zeros((0, 3), np.float32)
SMALL = (0, 1, 2, 3, 5)
EDGES = (0, 1, 5, 1024, 1025, 3000)
TORUS_ANGLE, OVERLAP_ANGLE = 5.0, 8.0


def torus_pair(angle=TORUS_ANGLE, n=1500):
    tgt, nrm = scan(n)
    perm = np.random.RandomState(77).permutation(n)
    return moved(tgt, motion(angle))[perm], tgt, nrm, perm


def overlap_pair():
    """(source, target, the true index of every overlap point): the part x > -0.3 of a 3 000-point target moved by
    OVERLAP_ANGLE, and 30 strays near (6, 6, 6)."""
    tgt, _ = scan(3000, 6)
    keep = np.flatnonzero(tgt[:, 0] > np.float32(-0.3))
    strays = (np.asarray([6.0, 6.0, 6.0]) + 0.1 * np.random.RandomState(8).uniform(-1, 1, (30, 3))).astype(np.float32)
    return np.concatenate([moved(tgt[keep], motion(OVERLAP_ANGLE)), strays]), tgt, keep


def sample_of(tgt, n, seed, angle=2.0):
    """n points of the target (with repetition), jittered and moved by ``angle``."""
    rng = np.random.RandomState(seed)
    P = tgt[rng.randint(0, tgt.shape[0], n)] + (0.5 * JITTER * rng.uniform(-1, 1, (n, 3))).astype(np.float32)
    return moved(P, motion(angle))


PYRAMID = dict(n=3000, angle=40.0, voxels=(0.2, 0.1, 0.02), factor=3.0, max_iter=50)


def part(n, seed=6):
    """An elliptical ring (semi-axes 1 and 0.6, tube 0.25) with a fifth of its points on a cap of radius 0.35 about
    (0.9, 0.3, 0.2), a jitter of JITTER: no symmetry, and a detail larger than the coarsest voxel of PYRAMID."""
    rng = np.random.RandomState(seed)
    u, v = rng.uniform(0, 2 * np.pi, n), rng.uniform(0, 2 * np.pi, n)
    nrm = np.stack([np.cos(v) * np.cos(u), np.cos(v) * np.sin(u), np.sin(v)], 1)
    P = np.stack([np.cos(u), 0.6 * np.sin(u), np.zeros(n)], 1) + 0.25 * nrm
    b = n // 5
    d = rng.normal(size=(b, 3))
    d[:, 2] = np.abs(d[:, 2])
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    P[:b] = np.asarray([0.9, 0.3, 0.2]) + 0.35 * d
    P = P + JITTER * rng.uniform(-1, 1, (n, 3))
    return P[rng.permutation(n)].astype(np.float32)


def pyramid_pair():
    """(source, target, perm): the part moved by PYRAMID's angle and row-permuted."""
    tgt = part(PYRAMID["n"])
    perm = np.random.RandomState(78).permutation(PYRAMID["n"])
    return moved(tgt, motion(PYRAMID["angle"]))[perm], tgt, perm


def line(n):
    k = np.arange(n, dtype=np.float64)[:, None]
    return (np.asarray([[1.0, 2.0, 3.0]]) + k * np.asarray([[0.125, 0.25, -0.125]])).astype(np.float32)


def flat(n, seed=9):
    rng = np.random.RandomState(seed)
    P = np.concatenate([rng.uniform(-1, 1, (n, 2)), np.full((n, 1), 0.25)], 1).astype(np.float32)
    return P, np.tile(np.asarray([[0.0, 0.0, 1.0]], np.float32), (n, 1))


def small_batch(mode):
    rng = np.random.RandomState(3)
    src, tgt, nrm = [], [], []
    for ns in SMALL:
        for nt in SMALL:
            T = rng.uniform(-1, 1, (nt, 3)).astype(np.float32)
            N = rng.normal(size=(nt, 3))
            src.append((T[rng.randint(0, max(nt, 1), ns)] if nt else rng.uniform(-1, 1, (ns, 3))).astype(np.float32)
                       + np.float32(0.01))
            tgt.append(T)
            nrm.append((N / np.maximum(np.linalg.norm(N, axis=1, keepdims=True), 1e-9)).astype(np.float32))
    return case(src, tgt, mode=mode, normals=nrm, max_iter=4)


def edge_batch(mode=POINT):
    tgt, nrm = scan(1500)
    return case([sample_of(tgt, n, 40 + n) for n in EDGES], [tgt] * len(EDGES), mode=mode, normals=[nrm] * len(EDGES),
                max_iter=4, max_dist=0.2)


def cases():
    """name -> the arguments of one call."""
    out = {}
    tgt, nrm = scan(1500)
    for mode, word in ((POINT, "point"), (PLANE, "plane")):
        out["small sizes, %s" % word] = small_batch(mode)
        for n in (1024, 1025, 2049):
            out["%d against 1500, %s" % (n, word)] = case(sample_of(tgt, n, n), tgt, mode=mode, normals=nrm, max_iter=5)
        out["tile edges batch, %s" % word] = edge_batch(mode)
    src, tgt, nrm, _ = torus_pair()
    out["torus, point"] = case(src, tgt, max_iter=30)
    out["torus, plane"] = case(src, tgt, mode=PLANE, normals=nrm, max_iter=30)
    out["torus, 20 degrees"] = case(torus_pair(20.0)[0], tgt, max_iter=30)
    osrc, otgt, _ = overlap_pair()
    out["partial overlap"] = case(osrc, otgt, max_dist=0.3, max_iter=30)
    out["line, point"] = case(moved(line(40), motion(3.0)), line(60), max_iter=6)
    P, N = flat(300)
    tilt = motion(4.0, shift=(0.01, 0.02, 0.03))
    out["plane with its normals, plane"] = case(moved(P[:200], motion(2.0)), P, mode=PLANE, normals=N, max_iter=6, init=tilt)
    out["mirrored source"] = case(src * np.asarray([1, 1, -1], np.float32), tgt, max_iter=6)
    nan_src = src.copy()
    nan_src[17, 1] = np.nan
    out["NaN source point"] = case(nan_src, tgt, max_iter=30)
    nan_tgt, inf_tgt, nan_nrm = tgt.copy(), tgt.copy(), nrm.copy()
    nan_tgt[5, 0], inf_tgt[1400, 2] = np.nan, -np.inf
    out["non-finite targets among clean ones"] = case([src[:300], src[:300], src[:300]], [nan_tgt, tgt, inf_tgt], max_iter=4)
    nan_nrm[np.arange(0, 1500, 7), 2] = np.nan
    out["NaN target normals"] = case(src, tgt, mode=PLANE, normals=nan_nrm, max_iter=30)
    out["init half a turn about z"] = case(src, tgt, max_iter=30, init=motion(180.0, (0, 0, 1), (0, 0, 0)))
    out["init the truth"] = case(src, tgt, max_iter=30, init=np.linalg.inv(motion(TORUS_ANGLE)))
    out["max_iter 1"] = case(src, tgt, max_iter=1)
    out["zero tolerances"] = case(src[:400], tgt, max_iter=12, tol=(0.0, 0.0))
    return out


# the names of ``cases()``, literally: a case cannot go missing without a test that says so
CASES = (
    "1024 against 1500, plane", "1024 against 1500, point", "1025 against 1500, plane", "1025 against 1500, point",
    "2049 against 1500, plane", "2049 against 1500, point", "NaN source point", "NaN target normals",
    "init half a turn about z", "init the truth", "line, point", "max_iter 1", "mirrored source",
    "non-finite targets among clean ones", "partial overlap", "plane with its normals, plane", "small sizes, plane",
    "small sizes, point", "tile edges batch, plane", "tile edges batch, point", "torus, 20 degrees", "torus, plane",
    "torus, point", "zero tolerances",
)


def test_the_case_list_is_literal():
    assert list(CASES) == sorted(cases())


_REFERENCE = {}


def reference_of(name):
    """register_numpy_batch of a case: computed once per process, shared (also with the GPU tests), never changed."""
    if name not in _REFERENCE:
        _REFERENCE[name] = register_numpy_batch(cases()[name])
    return _REFERENCE[name]


# ---------------------------------------------------------------------------------------------
# the host-compiled header
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    lib = native.build_harness(tmp_path_factory.mktemp("rrh"), "rrh", SOURCE)
    v, i, d, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_float
    lib.rrh_register.argtypes = [v, v, v, v, v, i, i, f, i, d, d, v, i, i, i, v, v, v, v, v, v, v]
    lib.rrh_apply.argtypes = [v, v, i, v, v]
    lib.rrh_pivot.restype = d
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def flat_case(c):
    """The arrays of a case as the C entry points take them."""
    S = len(c["src"])
    off_s = np.concatenate([[0], np.cumsum([x.shape[0] for x in c["src"]])]).astype(np.int32)
    off_t = np.concatenate([[0], np.cumsum([x.shape[0] for x in c["tgt"]])]).astype(np.int32)
    src = np.ascontiguousarray(np.concatenate([x.reshape(-1, 3) for x in c["src"]] + [EMPTY]), np.float32)
    tgt = np.ascontiguousarray(np.concatenate([x.reshape(-1, 3) for x in c["tgt"]] + [EMPTY]), np.float32)
    nrm = None if c["normals"] is None else np.ascontiguousarray(
        np.concatenate([x.reshape(-1, 3) for x in c["normals"]] + [EMPTY]), np.float32)
    init = None if c["init"] is None else np.ascontiguousarray(np.stack([np.asarray(m, np.float64).reshape(16)
                                                                         for m in c["init"]]))
    return S, src, off_s, tgt, off_t, nrm, init


def host_register(lib, c, order=0, sweeps=SWEEPS, ppc=4):
    S, src, off_s, tgt, off_t, nrm, init = flat_case(c)
    total = int(off_s[-1])
    T, rmse = np.full((S, 16), -9.0), np.full(S, -9.0)
    its, status, count = (np.full(S, -9, np.int32) for _ in range(3))
    idx, dist = np.full(total, -9, np.int32), np.full(total, -9, np.float32)
    rc = lib.rrh_register(_p(src), _p(off_s), _p(tgt), _p(off_t), _p(nrm), S, c["mode"], c["max_dist"], c["max_iter"],
                          c["tol"][0], c["tol"][1], _p(init), sweeps, order, ppc, _p(T), _p(its), _p(status), _p(count),
                          _p(rmse), _p(idx), _p(dist))
    assert rc == 12 + 9 * c["max_iter"]
    return T, its, status, count, rmse, idx, dist


def segment_of(c, s):
    return dict(c, src=[c["src"][s]], tgt=[c["tgt"][s]], normals=None if c["normals"] is None else [c["normals"][s]],
                init=None if c["init"] is None else [c["init"][s]])


def reversed_case(c):
    return dict(c, src=c["src"][::-1], tgt=c["tgt"][::-1], normals=None if c["normals"] is None else c["normals"][::-1],
                init=None if c["init"] is None else c["init"][::-1])


def rotation_defect(T):
    R = np.asarray(T, np.float64).reshape(4, 4)[:3, :3]
    return np.abs(R.T @ R - np.eye(3)).max()


def check_case(name, c, want):
    """What must hold of the definition's own result on the named case."""
    T, its, status, count, rmse, idx, dist = want
    for s in range(len(c["src"])):
        assert rotation_defect(T[s]) <= 1e-13 and np.linalg.det(T[s].reshape(4, 4)[:3, :3]) > 0, (name, s)
        assert 1 <= its[s] <= c["max_iter"] and (T[s, 12:] == [0, 0, 0, 1]).all()
    if name.startswith("small sizes"):
        need = 6 if c["mode"] == PLANE else 3
        for s, (ns, nt) in enumerate((a, b) for a in SMALL for b in SMALL):
            if ns < need or nt == 0:
                assert status[s] == TOO_FEW and its[s] == 1 and same(T[s], np.eye(4).reshape(16)), (ns, nt)
                assert count[s] == (ns if nt else 0) and (np.isnan(rmse[s]) if count[s] == 0 else rmse[s] >= 0)
        off = np.concatenate([[0], np.cumsum([a for a in SMALL for _ in SMALL])])
        for s, (ns, nt) in enumerate((a, b) for a in SMALL for b in SMALL):                  # an empty target: -1 / +inf
            rows = slice(off[s], off[s + 1])
            assert (idx[rows] == -1).all() == (nt == 0 or ns == 0) and np.isposinf(dist[rows]).all() == (nt == 0 or ns == 0)
    if name in ("torus, point", "torus, plane", "init the truth"):
        perm = torus_pair()[3]
        assert status[0] == CONVERGED and np.array_equal(idx, perm) and count[0] == 1500
        bound = 4 * math.sqrt(3) * 2.0 ** -24 * float(np.abs(np.concatenate([c["src"][0], c["tgt"][0]])).max())
        assert rmse[0] <= bound, (rmse[0], bound)
        back = T[0].reshape(4, 4) @ motion(TORUS_ANGLE)
        assert np.abs(back - np.eye(4)).max() <= 1e-6
        if name == "init the truth":
            assert its[0] == 1
    if name == "torus, 20 degrees":
        assert not np.array_equal(idx, torus_pair()[3])                      # a local minimiser: it needs a start
    if name == "partial overlap":
        keep = overlap_pair()[2]
        assert status[0] == CONVERGED and count[0] == keep.shape[0] and np.array_equal(idx[:-30][dist[:-30] <= 0.3], keep)
        assert (dist[-30:] > 0.3).all() and c["src"][0].shape[0] == keep.shape[0] + 30
    if name == "plane with its normals, plane":
        assert status[0] == DEGENERATE and its[0] == 1
        assert same(T[0].reshape(4, 4), matrix_of(*state_of(c["init"][0])))
    if name == "NaN source point":
        clean = reference_of("torus, point")
        assert idx[17] == -1 and np.isnan(dist[17]) and count[0] == 1499 and status[0] == CONVERGED
        assert np.array_equal(np.delete(idx, 17), np.delete(clean[5], 17))
    if name == "non-finite targets among clean ones":
        assert status.tolist()[0] == NON_FINITE == status[2] and status[1] != NON_FINITE and count.tolist()[0] == 0
        assert (idx[:300] == -1).all() and np.isnan(dist[:300]).all() and (idx[300:600] >= 0).all()
        assert same(T[0], np.eye(4).reshape(16)) and its[0] == 1
    if name == "NaN target normals":
        assert status[0] == CONVERGED and 0 < count[0] < 1500 and (idx % 7 != 0).sum() == count[0]
    if name == "max_iter 1":
        assert status[0] == MAX_ITER and its[0] == 1
    if name == "zero tolerances":
        assert status[0] in (MAX_ITER, CONVERGED)


@pytest.mark.parametrize("name", CASES)
def test_the_simulated_schedule_equals_the_definition(harness, name):
    c, want = cases()[name], reference_of(name)
    for order in (0, 1):
        got = host_register(harness, c, order)
        assert equal(got, want), (name, order, which_differ(got, want))
    check_case(name, c, want)


def test_plane_mode_needs_no_more_iterations_than_point_mode():
    point, plane = reference_of("torus, point"), reference_of("torus, plane")
    assert plane[2][0] == CONVERGED == point[2][0] and plane[1][0] <= point[1][0], (plane[1], point[1])


def test_half_a_turn_ends_in_a_local_minimum_the_truth_does_not():
    want = reference_of("init half a turn about z")
    assert want[2][0] in (CONVERGED, MAX_ITER) and not np.array_equal(want[5], torus_pair()[3])


@pytest.mark.parametrize("mode", (POINT, PLANE))
def test_a_segment_gives_the_same_bits_alone_in_a_batch_and_in_the_batch_reversed(harness, mode):
    name = "tile edges batch, %s" % ("plane" if mode == PLANE else "point")
    c, want = cases()[name], reference_of(name)
    back = host_register(harness, reversed_case(c))
    assert equal(back[:5], [w[::-1] for w in want[:5]])
    o = 0
    for s, n in enumerate(EDGES):
        alone = host_register(harness, segment_of(c, s))
        assert equal(alone, [w[s:s + 1] for w in want[:5]] + [w[o:o + n] for w in want[5:]]), (s, n)
        o += n
    assert want[2].tolist()[:2] == [TOO_FEW, TOO_FEW] and (want[3][3:] >= 1000).all()


def test_the_pyramid_reaches_the_true_pairs_where_one_level_does_not():
    """Both halves of tests/test_register_gpu.py's pyramid test on the restatement, before a GPU ever runs: coarse to
    fine over the voxel centroids of tests/test_voxel_abi.py's restatement the final transform pairs every source point
    with its true target point; ``register`` alone, from the same start and with the last level's max_dist, does not.
    The angle is 40 degrees: at 15 on this part (and on the torus at 10) one level alone still finds the pairs."""
    from tests.test_voxel_abi import voxel_numpy
    src, tgt, perm = pyramid_pair()
    f, voxels = PYRAMID["factor"], PYRAMID["voxels"]

    def centroids(P, h):
        out = voxel_numpy(P, h)
        return out[2][:out[1]]
    M = None
    for h in voxels:
        M = register_numpy(centroids(src, h), centroids(tgt, h), f * h, max_iter=PYRAMID["max_iter"], init=M)["transform"]
    assert np.array_equal(nearest_numpy(apply_numpy(src, M), tgt)[0], perm)
    one = register_numpy(src, tgt, f * voxels[-1], max_iter=PYRAMID["max_iter"])["transform"]
    assert not np.array_equal(nearest_numpy(apply_numpy(src, one), tgt)[0], perm)


def test_the_points_per_cell_move_no_bit(harness):
    c = cases()["1025 against 1500, point"]
    for ppc in (1, 32):
        assert equal(host_register(harness, c, ppc=ppc), reference_of("1025 against 1500, point")), ppc


def test_the_sweep_count_is_the_measured_one_plus_one(harness):
    """RR_SWEEPS - 1 is enough on every iteration of every point-mode case whose top eigenvalue is simple: one sweep
    more or fewer changes no bit."""
    for name in [n for n in CASES if cases()[n]["mode"] == POINT and n != "line, point"]:
        c = cases()[name]
        for sweeps in (SWEEPS - 1, SWEEPS + 1):
            got = host_register(harness, c, sweeps=sweeps)
            assert equal(got, reference_of(name)), (name, sweeps, which_differ(got, reference_of(name)))


def test_the_constants_are_the_ones_the_tests_assume(harness):
    assert [harness.rrh_constant(k) for k in range(8)] == [1024, SWEEPS, 256, CONVERGED, MAX_ITER, TOO_FEW, DEGENERATE,
                                                           NON_FINITE]
    assert harness.rrh_pivot() == PIVOT
    assert [harness.rrh_launches(m) for m in (0, 1, 2, 50, 256, 257, -1)] == [0, 21, 30, 462, 2316, 0, 0]


def test_the_move_step_alone(harness):
    src = cases()["torus, point"]["src"][0]
    for M in (motion(33.0), motion(180.0, (0, 0, 1)), motion(179.0, (1, 0, 0)), motion(120.0, (1, 1, 1)), np.eye(4)):
        out = np.zeros_like(src)
        off = np.asarray([0, src.shape[0]], np.int32)
        harness.rrh_apply(_p(src), _p(off), 1, _p(np.ascontiguousarray(M.reshape(16))), _p(out))
        assert same(out, apply_numpy(src, M))
        assert np.abs(out - moved(src, M)).max() <= 4 * 2.0 ** -24 * (np.abs(src).max() + 1)      # it is the motion
        assert np.abs(matrix_of(*state_of(M)) - M).max() <= 1e-15 * 8                               # the extraction rule


def test_the_program_under_the_sanitizers_over_the_case_list(tmp_path):
    """The same file with its main, built with -fsanitize=address,undefined (the runtimes linked into the program) and
    run over every case of ``cases()`` from a file, in both orders of the tiles.  It runs in the environment it finds:
    nothing is preloaded or set for it."""
    exe = os.path.join(str(tmp_path), "register_host")
    subprocess.run(native.GXX + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                                 "-static-libubsan", "-o", exe, SOURCE], check=True)
    names = sorted(cases())
    path = tmp_path / "cases.txt"
    with open(path, "w") as f:
        for name in names:
            c = cases()[name]
            f.write("%d %d %.9g %d %.17g %.17g %d %d\n" % (len(c["src"]), c["mode"], np.float32(c["max_dist"]),
                                                            c["max_iter"], c["tol"][0], c["tol"][1],
                                                            c["normals"] is not None, c["init"] is not None))
            for s in range(len(c["src"])):
                f.write("%d %d\n" % (c["src"][s].shape[0], c["tgt"][s].shape[0]))
                if c["init"] is not None:
                    f.write(" ".join("%.17g" % v for v in np.asarray(c["init"][s], np.float64).reshape(16)) + "\n")
                f.write("".join("%.9g %.9g %.9g\n" % tuple(p) for p in c["src"][s].tolist()))
                rows = c["tgt"][s] if c["normals"] is None else np.concatenate([c["tgt"][s], c["normals"][s]], 1)
                f.write("".join(" ".join("%.9g" % v for v in p) + "\n" for p in rows.tolist()))
    run = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-2000:]
    words = iter(run.stdout.split())
    for name in names:
        c, want = cases()[name], reference_of(name)
        o = 0
        for s in range(len(c["src"])):
            assert same(np.asarray([float(next(words)) for _ in range(16)]), want[0][s]), name
            assert [int(next(words)) for _ in range(3)] == [want[1][s], want[2][s], want[3][s]], name
            assert same(np.float64(next(words)), want[4][s]), name
            n = c["src"][s].shape[0]
            rows = [(int(next(words)), np.float32(next(words))) for _ in range(n)]
            assert same(np.asarray([r[0] for r in rows], np.int32).reshape(-1), want[5][o:o + n]), name
            assert same(np.asarray([r[1] for r in rows], np.float32).reshape(-1), want[6][o:o + n]), name
            o += n
    assert next(words, None) is None


# ---------------------------------------------------------------------------------------------
# the exports, the schedule, the workspace and the argument checks, which run before anything touches a GPU
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    return native.load_raw(NAMES)


def test_the_entry_points_are_exported_and_bound(lib, harness):
    from parsenet_codebase_amd import _lib
    v, i, ll, d, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_double, ctypes.c_float
    assert _lib.SIGNATURES["pn_register_f32"] == (i, [v, v, i, v, v, i, v, i, i, f, i, d, d, v, v, v, v, v, v, v, v, v, ll, v])
    assert _lib.SIGNATURES["pn_register_workspace_bytes"] == (ll, [ll, ll, i])
    assert _lib.SIGNATURES["pn_register_launches"] == (i, [i])
    assert _lib.SIGNATURES["pn_rigid_apply_f32"] == (i, [v, v, i, i, v, v, v])
    assert lib.pn_abi_version() == 23 == _lib.CONSTANTS["PN_ABI_VERSION"]                   # added symbols only
    assert all(hasattr(_lib.load(), n) for n in NAMES)
    for m in (-1, 0, 1, 2, 30, 50, 256, 257):                                               # 12 + 9 max_iter
        assert lib.pn_register_launches(m) == harness.rrh_launches(m) == (12 + 9 * m if 1 <= m <= 256 else 0), m
    w = lib.pn_register_workspace_bytes
    for totalS, totalT, S in ((1, 1, 1), (1024, 3000, 3), (10 ** 6, 10 ** 6, 4), (0, 5, 2), (5, 0, 2)):
        query = lib.pn_knn3_query_workspace_bytes(totalT, totalS, S) - 16
        assert w(totalS, totalT, S) == query + 20 * totalS + 236 * (totalS // 1024 + S) + 120 * S + 16
    assert w(-1, 1, 1) == 0 and w(1, -1, 1) == 0 and w(1, 1, -1) == 0 and w(2 ** 31, 1, 1) == 0


ARGS = ("src", "off_s", "totalS", "tgt", "off_t", "totalT", "normals", "S", "mode", "max_dist", "max_iter", "tol_rot",
        "tol_trans", "init", "transform", "iterations", "status", "count", "rmse", "idx", "dist", "ws", "ws_bytes",
        "stream")


def raw_call(lib, **over):
    """pn_register_f32 with plausible arguments (never dereferenced by a call that is refused), some replaced."""
    a = dict(src=64, off_s=64, totalS=10, tgt=64, off_t=64, totalT=10, normals=None, S=1, mode=0, max_dist=1.0,
             max_iter=5, tol_rot=1e-6, tol_trans=1e-6, init=None, transform=64, iterations=64, status=64, count=64,
             rmse=64, idx=None, dist=None, ws=64, ws_bytes=lib.pn_register_workspace_bytes(10, 10, 1), stream=None)
    a.update(over)
    return lib.pn_register_f32(*[a[n] for n in ARGS])


def test_invalid_arguments_are_refused_before_any_launch(lib):
    """(No GPU is needed to get here: a refused call, and one with nothing to do, launch nothing.)"""
    from parsenet_codebase_amd import _lib
    err = _lib.CONSTANTS["PN_ERR_ARG"]
    need = lib.pn_register_workspace_bytes(10, 10, 1)
    for over, word in ((dict(S=-1), b"S=-1"), (dict(totalS=-1), b"totalS=-1"), (dict(totalT=-1), b"totalT=-1"),
                       (dict(mode=2), b"mode=2"), (dict(mode=-1), b"mode=-1"), (dict(mode=1), b"normals"),
                       (dict(max_iter=0), b"max_iter=0"), (dict(max_iter=257), b"max_iter=257"),
                       (dict(max_dist=-1.0), b"max_dist"), (dict(max_dist=float("nan")), b"max_dist"),
                       (dict(tol_rot=-1.0), b"tol_rot"), (dict(tol_trans=float("nan")), b"tol_trans"),
                       (dict(src=None), b"null"), (dict(off_s=None), b"null"), (dict(tgt=None), b"null"),
                       (dict(off_t=None), b"null"), (dict(transform=None), b"null"), (dict(iterations=None), b"null"),
                       (dict(status=None), b"null"), (dict(count=None), b"null"), (dict(rmse=None), b"null"),
                       (dict(ws=None), b"null"), (dict(ws_bytes=need - 1), b"workspace"), (dict(ws_bytes=0), b"workspace")):
        assert raw_call(lib, **over) == err, over
        assert b"pn_register_f32" in lib.pn_last_error() and word in lib.pn_last_error(), (over, lib.pn_last_error())
    assert raw_call(lib, S=0) == 0 and raw_call(lib, S=0, src=None, tgt=None, transform=None, ws=None, ws_bytes=0) == 0
    assert raw_call(lib, S=0, max_iter=0) == err and raw_call(lib, S=0, mode=7) == err      # the arguments come first
    assert lib.pn_rigid_apply_f32(None, 64, 1, 10, 64, 64, None) == err and b"pn_rigid_apply_f32" in lib.pn_last_error()
    assert lib.pn_rigid_apply_f32(64, 64, -1, 10, 64, 64, None) == err and lib.pn_rigid_apply_f32(64, 64, 1, -1, 64, 64, None) == err
    assert lib.pn_rigid_apply_f32(64, 64, 0, 10, 64, 64, None) == 0 and lib.pn_rigid_apply_f32(None, 64, 1, 0, None, 64, None) == 0


def test_python_argument_checks_need_no_gpu():
    import torch
    from parsenet_codebase_amd import kernels, registration
    P = torch.zeros(8, 3)
    off = torch.tensor([0, 8], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="MI355X only"):
        kernels.register_ragged(P, off, P, off, 0.1)
    with pytest.raises(RuntimeError, match="MI355X only"):
        kernels.rigid_apply(P, off, torch.eye(4, dtype=torch.float64)[None])
    for over, word in ((dict(max_dist=-1.0), "max_dist"), (dict(max_dist=float("nan")), "max_dist"),
                       (dict(max_dist="a"), "max_dist"), (dict(max_dist=True), "max_dist"),
                       (dict(method="both"), "method"), (dict(method="plane"), "target_normals"),
                       (dict(max_iter=0), "max_iter"), (dict(max_iter=257), "max_iter"), (dict(max_iter=1.5), "max_iter"),
                       (dict(max_iter=True), "max_iter"), (dict(tol_rot=-1e-3), "tol_rot"),
                       (dict(tol_trans=float("nan")), "tol_trans"), (dict(init=torch.eye(3)), "init"),
                       (dict(init=torch.eye(4)), "init"), (dict(init=[[1.0]]), "init"),
                       (dict(method="point", target_normals=P), "target_normals")):
        with pytest.raises((ValueError, TypeError), match=word):
            registration.register(P, P, **dict(dict(max_dist=0.1), **over))
    with pytest.raises(RuntimeError, match="MI355X only"):
        registration.register(P, P, 0.1)
    for voxels in ([], [0.1, -1.0], [float("inf")], "ab", 0.1):
        with pytest.raises(ValueError, match="voxels"):
            registration.register_pyramid(P, P, voxels)
    for factor in (0.0, -1.0, True, "3"):
        with pytest.raises(ValueError, match="max_dist_factor"):
            registration.register_pyramid(P, P, [0.1], max_dist_factor=factor)
    with pytest.raises(ValueError, match="max_dist follows"):
        registration.register_pyramid(P, P, [0.1], max_dist=0.3)
    with pytest.raises(RuntimeError, match="MI355X only"):
        registration.register_pyramid(P, P, [0.1])
    with pytest.raises(RuntimeError, match="MI355X only"):
        registration.apply_transform(P, torch.eye(4, dtype=torch.float64))
    assert registration.STATUS_NAMES == {0: "converged", 1: "max_iter", 2: "too_few", 3: "degenerate", 4: "non_finite"}
