"""CPU-side checks of the consistent normal orientation without a viewpoint (csrc/orient_math.h, csrc/orient.hip): the
header's weight, sign and keys on hand-made pairs; the serial restatement compiled for the host
(tests/native/orient_math_host.cpp: Kruskal, tree walk, seed rule) against an independent restatement in numpy/Python
on every input of this file, exactly; the quality condition — every oriented normal of four closed shapes has a
positive dot with the analytic outward normal, at k = 8 and 16; the exact cases; the stand-alone program; the export
of pn_orient_normals_f32 and its argument checks."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests.helpers import native
from tests.helpers.native import ROOT
from tests.test_point_normals_abi import knn3, reference, sphere

SOURCE = native.source("orient_math_host.cpp")
NAME = "pn_orient_normals_f32"
ARGS = ("pts", "off", "S", "total", "idx", "k", "normals_in", "normals_out", "flip", "seed", "stream")


# ---------------------------------------------------------------------------------------------
# inputs: closed shapes with their analytic outward normals
# ---------------------------------------------------------------------------------------------
def two_spheres():
    """300 points at radius 1 at the origin and 200 at radius 0.5 at (5, 0, 0.3): the k-NN graph falls into two parts."""
    a, b = sphere(300).astype(np.float64), sphere(200).astype(np.float64)
    pts = np.concatenate([a, 0.5 * b + np.asarray([5.0, 0.0, 0.3])])
    return pts.astype(np.float32), np.concatenate([a, b])


def torus(R=0.7, r=0.25, nu=60, nv=25, seed=4):
    """1 500 points of a jittered nu x nv grid (a quarter of a cell either way) on the torus around the z axis."""
    rng = np.random.RandomState(seed)
    u, v = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    u = 2 * np.pi * (u + 0.25 * rng.uniform(-1, 1, u.shape)).reshape(-1) / nu
    v = 2 * np.pi * (v + 0.25 * rng.uniform(-1, 1, v.shape)).reshape(-1) / nv
    out = np.stack([np.cos(v) * np.cos(u), np.cos(v) * np.sin(u), np.sin(v)], 1)
    pts = np.stack([R * np.cos(u), R * np.sin(u), np.zeros_like(u)], 1) + r * out
    return pts.astype(np.float32), out


def capsule(n_caps=800, n_around=40, n_along=10, height=1.2, scale=0.4, seed=6):
    """A capsule with a tilted axis: the 800-point spiral sphere split at its equator into two caps, moved apart along
    the axis by ``height``, and a 400-point jittered band of the unit cylinder between them; scaled by 0.4."""
    rng = np.random.RandomState(seed)
    s = sphere(n_caps).astype(np.float64)
    caps = s + np.where(s[:, 2:] >= 0, 0.5, -0.5) * np.asarray([0.0, 0.0, height])
    a, h = np.meshgrid(np.arange(n_around), np.arange(n_along), indexing="ij")
    a = 2 * np.pi * (a + 0.5 * (h % 2) + 0.2 * rng.uniform(-1, 1, a.shape)).reshape(-1) / n_around
    h = height * ((h + 0.5 + 0.2 * rng.uniform(-1, 1, h.shape)).reshape(-1) / n_along - 0.5)
    radial = np.stack([np.cos(a), np.sin(a), np.zeros_like(a)], 1)
    pts = np.concatenate([caps, radial + h[:, None] * np.asarray([0.0, 0.0, 1.0])])
    out = np.concatenate([s, radial])
    ax = np.asarray([0.3, -0.5, 0.81])
    ax /= np.linalg.norm(ax)
    e1 = np.cross(ax, [1.0, 0.0, 0.0])
    e1 /= np.linalg.norm(e1)
    rot = np.stack([e1, np.cross(ax, e1), ax], 1)          # columns: the images of x, y, z
    return (scale * pts @ rot.T + np.asarray([0.1, 0.2, -0.05])).astype(np.float32), out @ rot.T


def closed_shapes():
    s = sphere()
    return {"sphere 500": (s, s.astype(np.float64)), "two spheres": two_spheres(), "torus": torus(),
            "tilted capsule": capsule()}


def canonical_normals(P, idx):
    """float64 eigh normals of the neighbourhoods, rounded to fp32, canonical sign: the component of largest magnitude
    positive (the lowest axis on a tie) — what estimate_normals gives without a viewpoint."""
    n = reference(P, idx)[0].astype(np.float32)
    lead = n[np.arange(n.shape[0]), np.argmax(np.abs(n), 1)]
    return np.where((lead < 0)[:, None], -n, n)


# ---------------------------------------------------------------------------------------------
# the independent restatement: numpy keys, Kruskal with union-find, breadth-first walk
# ---------------------------------------------------------------------------------------------
def py_weights(normals, idx):
    """(w (n,k) fp32, neg (n,k) bool, valid (n,k) bool) of every entry."""
    n, k = idx.shape
    a = normals.astype(np.float64)[:, None, :]
    valid = (idx != np.arange(n)[:, None]) & (idx >= 0) & (idx < n)
    b = normals.astype(np.float64)[np.where(valid, idx, 0)]
    dot = (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
    d = 1.0 - np.abs(dot)
    return np.where(d > 0, d, 0.0).astype(np.float32), dot < 0, valid


def py_orient(P, idx, normals):
    """(oriented normals, flip, seed) of one cloud by the definition of csrc/orient_math.h."""
    P, normals, idx = np.asarray(P, np.float32), np.asarray(normals, np.float32), np.asarray(idx, np.int32)
    n, k = idx.shape
    w, neg, valid = py_weights(normals, idx)
    entry = np.arange(n * k, dtype=np.uint64).reshape(n, k)
    keys = np.sort(((w.view(np.uint32).astype(np.uint64) << np.uint64(32)) | entry)[valid])
    parent = list(range(n))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v

    adj = [[] for _ in range(n)]
    for e in (keys & np.uint64(0xffffffff)).astype(np.int64).tolist():
        i, j = e // k, int(idx.reshape(-1)[e])
        a, b = find(i), find(j)
        if a != b:
            parent[max(a, b)] = min(a, b)
            sign = bool(neg.reshape(-1)[e])
            adj[i].append((j, sign))
            adj[j].append((i, sign))
    root = np.asarray([find(v) for v in range(n)], np.int64)
    z = P[:, 2] + np.float32(0.0)
    flip, seed = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    for r in np.unique(root):
        members = np.flatnonzero(root == r)
        sd = int(members[np.argmax(z[members])])           # the first of the largest: the lowest index
        flip[sd], seed[sd] = int(normals[sd, 2] < 0), sd
        queue = [sd]
        while queue:
            v = queue.pop()
            for u, sign in adj[v]:
                if flip[u] < 0:
                    flip[u], seed[u] = flip[v] ^ int(sign), sd
                    queue.append(u)
    return np.where((flip == 1)[:, None], -normals, normals), flip, seed


# ---------------------------------------------------------------------------------------------
# the host-compiled restatement
# ---------------------------------------------------------------------------------------------
def build_harness(directory):
    lib = native.build_harness(directory, "omh", SOURCE)
    lib.omh_weight.restype = ctypes.c_float
    lib.omh_weight.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.omh_key.restype = lib.omh_zkey.restype = ctypes.c_ulonglong
    lib.omh_key.argtypes = lib.omh_zkey.argtypes = [ctypes.c_float, ctypes.c_uint]
    return lib


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory.mktemp("omh"))


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def host_orient(harness, P, off, idx, normals):
    """(oriented normals (total,3) fp32, flip, seed int32) of the host compile over a ragged batch."""
    P, normals = np.ascontiguousarray(P, np.float32), np.ascontiguousarray(normals, np.float32)
    off, idx = np.ascontiguousarray(off, np.int32), np.ascontiguousarray(idx, np.int32)
    total, k = idx.shape
    out = np.full((total, 3), np.nan, np.float32)
    flip, seed = np.full(total, -7, np.int32), np.full(total, -7, np.int32)
    harness.omh_orient(_p(P), _p(off), off.shape[0] - 1, _p(idx), k, _p(normals), _p(out), _p(flip), _p(seed))
    return out, flip, seed


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def both(harness, P, idx, normals):
    """The two restatements on one cloud, which must agree in every bit; returns (normals, flip, seed)."""
    P, normals = np.asarray(P, np.float32), np.asarray(normals, np.float32)
    got = host_orient(harness, P, [0, P.shape[0]], idx, normals)
    want = py_orient(P, idx, normals)
    assert same_bits(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert set(np.unique(got[1]).tolist()) <= {0, 1}
    assert same_bits(got[0], np.where((got[1] == 1)[:, None], -normals, normals))    # the input, or exactly negated
    return got


# ---------------------------------------------------------------------------------------------
# the header on hand-made pairs
# ---------------------------------------------------------------------------------------------
def _weight(harness, a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    neg = np.full(1, -1, np.int32)
    w = harness.omh_weight(_p(a), _p(b), _p(neg))
    return w, int(neg[0])


def test_weight_sign_and_keys_on_hand_made_pairs(harness):
    assert _weight(harness, [0, 0, 1], [0, 0, 1]) == (0.0, 0)                      # parallel
    assert _weight(harness, [0, 0, 1], [0, 0, -1]) == (0.0, 1)                     # antiparallel
    assert _weight(harness, [1, 0, 0], [0, 1, 0]) == (1.0, 0)                      # orthogonal: dot == 0 is not negative
    assert _weight(harness, [0, 0, 0], [0.6, 0, 0.8]) == (1.0, 0)                  # a zero normal
    assert _weight(harness, [0, 0, 0], [0, 0, 0]) == (1.0, 0)
    assert _weight(harness, [0.5, 0.5, 0], [0.5, 0, 0]) == (0.75, 0)
    assert _weight(harness, [0.5, 0.5, 0], [-0.5, 0, 0]) == (0.75, 1)
    assert _weight(harness, [2, 0, 0], [3, 0, 0]) == (0.0, 0)                      # |dot| > 1: clamped to 0
    # fp64 on the fp32 values, ((xx + yy) + zz): 1 - (1 - 2^-24)^2 = 2^-23 - 2^-48 is kept, and rounds to fp32 once
    a = np.asarray([1 - 2.0 ** -24, 0, 0], np.float32)
    assert _weight(harness, a, a) == (float(np.float32(2.0 ** -23 - 2.0 ** -48)), 0)
    # bitwise symmetric in its arguments, on random pairs
    rng = np.random.RandomState(0)
    for a, b in rng.standard_normal((200, 2, 3)).astype(np.float32) * 0.6:
        assert _weight(harness, a, b) == _weight(harness, b, a)
    # the key: the weight's bits above the entry index, so that keys order as (w, entry) does
    assert harness.omh_key(0.0, 5) == 5 and harness.omh_key(1.0, 0) == 0x3f800000 << 32
    assert harness.omh_key(0.25, 7) == (0x3e800000 << 32) | 7
    assert harness.omh_key(0.25, 0xffffffff) < harness.omh_key(np.nextafter(np.float32(0.25), np.float32(1)), 0)
    # the seed order: larger z first, -0 as +0, then the LOWER index
    zk = harness.omh_zkey
    assert zk(1.0, 9) > zk(0.5, 0) > zk(0.0, 0) > zk(-0.5, 0) > zk(-1.0, 0)
    assert zk(0.25, 3) > zk(0.25, 4) and zk(-0.0, 3) == zk(0.0, 3)


def test_python_weights_are_the_headers(harness):
    P = sphere(60)
    idx = knn3(P, 5)
    nrm = canonical_normals(P, idx)
    w, neg, valid = py_weights(nrm, idx)
    assert valid[:, 1:].all() and not valid[:, 0].any()
    for i in range(P.shape[0]):
        for s in range(1, 5):
            assert _weight(harness, nrm[i], nrm[idx[i, s]]) == (float(w[i, s]), int(neg[i, s]))


# ---------------------------------------------------------------------------------------------
# the quality condition
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (8, 16))
def test_every_oriented_normal_of_a_closed_shape_points_outward(harness, k):
    """Canonical-sign normals agree with the outward normal at about half of the points; oriented, at every point."""
    for name, (P, outward) in closed_shapes().items():
        idx = knn3(P, k)
        nrm = canonical_normals(P, idx)
        before = float(((nrm.astype(np.float64) * outward).sum(1) > 0).mean())
        got, flip, seed = both(harness, P, idx, nrm)
        after = (got.astype(np.float64) * outward).sum(1) > 0
        print("%s, k = %d: %d points, outward before %.3f, after %.3f, %d seed(s)"
              % (name, k, P.shape[0], before, after.mean(), np.unique(seed).size))
        assert 0.3 < before < 0.7, (name, k, before)
        assert after.all(), (name, k, float(after.mean()))
        assert np.unique(seed).size == (2 if name == "two spheres" else 1), name
    # the two spheres: each part has its own seed, its topmost point
    P, _ = two_spheres()
    _, _, seed = both(harness, P, knn3(P, k), canonical_normals(P, knn3(P, k)))
    assert set(seed[:300].tolist()) == {int(np.argmax(P[:300, 2]))}
    assert set(seed[300:].tolist()) == {300 + int(np.argmax(P[300:, 2]))}


# ---------------------------------------------------------------------------------------------
# exact cases
# ---------------------------------------------------------------------------------------------
def lattice(nx=8, ny=9, z=0.375):
    """A dyadic planar lattice: every coordinate a multiple of 1/8."""
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    return np.stack([i.reshape(-1) / 8.0, j.reshape(-1) / 8.0, np.full(nx * ny, z)], 1).astype(np.float32)


UP = np.asarray([0, 0, 1], np.float32)


def test_all_ties_lattice(harness):
    """Identical normals: every weight is 0 and the entry index alone decides the tree."""
    P = lattice()
    n = P.shape[0]
    for k in (5, 16):
        idx = knn3(P, k)
        got, flip, seed = both(harness, P, idx, np.tile(UP, (n, 1)))
        assert same_bits(got, np.tile(UP, (n, 1))) and not flip.any() and not seed.any()    # equal z: the lowest index
        # half of the normals negated on input: all come out +z
        down = np.random.RandomState(k).permutation(n) < n // 2
        for mask in (down, ~down):
            got, flip, seed = both(harness, P, idx, np.where(mask[:, None], -UP, UP))
            assert np.array_equal(got, np.tile(UP, (n, 1))) and np.array_equal(flip == 1, mask) and not seed.any()


def test_duplicated_points(harness):
    base, _ = torus(nu=12, nv=8)
    P = np.concatenate([base, base])[np.random.RandomState(1).permutation(2 * base.shape[0])]
    for k in (3, 8):
        idx = knn3(P, k)
        nrm = canonical_normals(P, knn3(P, 12))
        got, flip, seed = both(harness, P, idx, nrm)
        assert (seed >= 0).all() and (seed[seed] == seed).all()


def test_tiny_clouds_and_padding(harness):
    one = np.asarray([[0.5, 0.25, -1.0]], np.float32)
    for nz, f in ((1.0, 0), (-1.0, 1)):
        got, flip, seed = both(harness, one, knn3(one, 4), np.asarray([[0, 0, nz]], np.float32))
        assert got.tolist() == [[0, 0, 1]] and flip.tolist() == [f] and seed.tolist() == [0]
    two = np.asarray([[0, 0, 0], [0.5, 0, 0.25]], np.float32)
    assert knn3(two, 5).tolist() == [[0, 1, 0, 0, 0], [1, 0, 1, 1, 1]]                      # padded with the point itself
    got, flip, seed = both(harness, two, knn3(two, 5), np.asarray([[0, 0.6, 0.8], [0, -0.6, -0.8]], np.float32))
    assert got.tolist() == [[0, np.float32(0.6), np.float32(0.8)]] * 2 and flip.tolist() == [0, 1]
    assert seed.tolist() == [1, 1]
    # k = 1: no entry, every point its own component and seed
    P = lattice(3, 3)
    nrm = np.tile(-UP, (9, 1))
    got, flip, seed = both(harness, P, knn3(P, 1), nrm)
    assert np.array_equal(got, -nrm) and flip.all() and seed.tolist() == list(range(9))
    # n < k on a real cloud
    P = sphere(7)
    for k in (8, 16, 64):
        idx = knn3(P, k)
        assert (idx[:, 7:] == np.arange(7)[:, None]).all()
        _, _, seed = both(harness, P, idx, canonical_normals(P, knn3(P, 7)))
        assert not seed.any()                                                                # the spiral starts on top
    # an index outside the segment is dropped like a self entry: no read leaves the cloud
    idx = knn3(P, 4)
    wild = idx.copy()
    wild[:, 3] = np.where(np.arange(7) % 2 == 0, -1, 7)
    nrm = canonical_normals(P, knn3(P, 7))
    cut = idx.copy()
    cut[:, 3] = np.arange(7)
    a, b = both(harness, P, wild, nrm), both(harness, P, cut, nrm)
    assert same_bits(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_zero_normals_and_a_level_seed(harness):
    P = sphere(50)
    idx = knn3(P, 6)
    got, flip, seed = both(harness, P, idx, np.zeros((50, 3), np.float32))
    assert not got.any() and not np.signbit(got).any() and not flip.any() and not seed.any()
    # a zero normal among real ones takes its neighbours' flip and stays zero
    nrm = canonical_normals(P, idx)
    nrm[20] = 0
    got, flip, _ = both(harness, P, idx, nrm)
    assert not got[20].any() and (np.delete(got, 20, 0).astype(np.float64) * np.delete(P, 20, 0)).sum(1).min() > 0
    # a seed with n_z == 0 (+0, -0, the zero normal) keeps flip = 0, whatever its other components
    P = lattice(4, 4)
    P[5, 2] = 0.5                                                                            # the topmost point
    idx = knn3(P, 5)
    for nz in (0.0, -0.0):
        for nx in (1.0, -1.0):
            nrm = np.tile(np.asarray([nx, 0, nz], np.float32), (16, 1))
            got, flip, seed = both(harness, P, idx, nrm)
            assert (seed == 5).all() and not flip.any() and same_bits(got, nrm)
    nrm = np.tile(-UP, (16, 1))
    nrm[5] = 0
    got, flip, seed = both(harness, P, idx, nrm)                # w = 1 to the zero seed, neg = false: nobody flips
    assert (seed == 5).all() and not flip.any()
    P[5, 2], P[9, 2] = -0.0, 0.0                                 # -0 == +0: the lowest index among equal z
    P[:, 2] = np.where(np.isin(np.arange(16), (5, 9)), P[:, 2], -1.0)
    assert (both(harness, P, idx, np.tile(UP, (16, 1)))[2] == 5).all()


def test_the_program_reads_a_cloud_from_stdin_and_a_file(harness, tmp_path):
    exe = native.build_program(tmp_path, "orient_math_host", SOURCE)
    P, _ = torus(nu=16, nv=9)
    k = 6
    idx = knn3(P, k)
    nrm = canonical_normals(P, idx)
    text = "%d %d\n" % (P.shape[0], k) + "".join("%.9g %.9g %.9g %.9g %.9g %.9g\n" % (tuple(p) + tuple(n))
                                                  for p, n in zip(P, nrm))
    text += "".join(" ".join(str(j) for j in row) + "\n" for row in idx)
    path = tmp_path / "torus.txt"
    path.write_text(text)
    want = both(harness, P, idx, nrm)
    for run in (subprocess.run([exe], input=text, capture_output=True, text=True, check=True),
                subprocess.run([exe, str(path)], capture_output=True, text=True, check=True)):
        rows = [line.split() for line in run.stdout.splitlines()]
        assert np.array_equal(np.asarray([[float(x) for x in r[:3]] for r in rows], np.float32), want[0])
        assert [int(r[3]) for r in rows] == want[1].tolist() and [int(r[4]) for r in rows] == want[2].tolist()
    assert subprocess.run([exe], input="5 0\n", capture_output=True, text=True).returncode == 2
    assert subprocess.run([exe], input="2 2\n0 0 0 0 0 1\n", capture_output=True, text=True).returncode == 2


# ---------------------------------------------------------------------------------------------
# the export and the argument checks, which run before anything touches a GPU
# ---------------------------------------------------------------------------------------------
def load_raw():
    return native.load_raw((NAME, "pn_orient_normals_max_points"))


@pytest.fixture(scope="module")
def lib():
    return load_raw()


def test_the_entry_point_is_exported_and_bound(lib):
    from parsenet_codebase_amd import _lib
    v, i = ctypes.c_void_p, ctypes.c_int
    assert _lib.SIGNATURES[NAME] == (i, [v, v, i, i, v, i, v, v, v, v, v])
    assert _lib.SIGNATURES["pn_orient_normals_max_points"] == (i, [])
    assert 1024 <= lib.pn_orient_normals_max_points() <= 10240
    assert lib.pn_abi_version() == 23 == _lib.CONSTANTS["PN_ABI_VERSION"]                   # an added symbol
    assert [line for line in open(os.path.join(ROOT, "include", "parsenet_hip.h")) if NAME + "(" in line]


def raw_call(lib, **over):
    """pn_orient_normals_f32 with plausible arguments (never dereferenced by a call that is refused), some replaced."""
    a = dict(pts=64, off=64, S=1, total=10, idx=64, k=8, normals_in=64, normals_out=128, flip=None, seed=None,
             stream=None)
    a.update(over)
    return lib.pn_orient_normals_f32(*[a[n] for n in ARGS])


def check_invalid_arguments(lib, **real):
    """k out of range, S < 0, total < 0, a null required pointer, output on input: PN_ERR_ARG; nothing to do: 0."""
    from parsenet_codebase_amd import _lib
    err = _lib.CONSTANTS["PN_ERR_ARG"]
    alias = dict(normals_out=real.get("normals_in", 64))
    for over in (dict(k=0), dict(k=65), dict(k=-3), dict(S=-1), dict(total=-1), dict(pts=None), dict(off=None),
                 dict(idx=None), dict(normals_in=None), dict(normals_out=None), alias):
        assert raw_call(lib, **dict(real, **over)) == err, over
        assert b"pn_orient_normals_f32" in lib.pn_last_error()
    assert raw_call(lib, **dict(real, total=0)) == 0
    assert raw_call(lib, **dict(real, S=0)) == 0
    assert raw_call(lib, **dict(real, total=0, pts=None, idx=None, normals_in=None, normals_out=None)) == 0


def test_invalid_arguments_are_refused_before_any_launch(lib):
    """(No GPU is needed to get here: a refused call, and one with nothing to do, launch nothing.)"""
    check_invalid_arguments(lib)


def test_python_argument_checks_need_no_gpu():
    import torch
    from parsenet_codebase_amd import kernels, point_normals
    z = torch.zeros(8, 3)
    with pytest.raises(RuntimeError, match="MI355X only"):
        point_normals.orient_normals(z, z)
    with pytest.raises(RuntimeError, match="MI355X only"):
        kernels.orient_normals(z, [0, 8], torch.zeros(8, 3, dtype=torch.int32), 3, z)
    with pytest.raises(TypeError):
        point_normals.orient_normals(np.zeros((8, 3), np.float32), z)
    with pytest.raises(ValueError, match="empty list"):
        point_normals.orient_normals([], [])
    with pytest.raises(ValueError, match="orient must be"):
        point_normals.estimate_normals(z, orient="bfs")
    with pytest.raises(ValueError, match="orient must be"):
        point_normals.estimate_normals(z, orient=True)
    with pytest.raises(ValueError, match="viewpoint"):
        point_normals.estimate_normals(z, orient="mst", viewpoint=torch.zeros(3))
    with pytest.raises(RuntimeError, match="MI355X only"):
        point_normals.estimate_normals(z, orient="mst")
