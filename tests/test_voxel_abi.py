"""CPU-side checks of the voxel-grid downsampling: csrc/voxel_math.h compiled for the host into a serial restatement of
the kernels' schedule (tests/native/voxel_host.cpp: bounds, the open-addressing table, heads, the scan of the tile
counts, voxel rows, owner, rep) against ``voxel_numpy``, an independent numpy restatement of the definition (a dict from
the cell triple to its members, the sums in Python integers, np.float32 arithmetic for the distances) — every output
exactly equal, with two table capacities and both orders of arrival —, the exact properties of the definition, the
stand-alone program, the export of csrc/voxel.hip and its argument checks."""
import ctypes
import math
import subprocess

import numpy as np
import pytest

from tests.helpers import native
from tests.test_fps_abi import same
from tests.test_knn3_grid_abi import collinear, copies_among_random, lattice, offset_cloud, planar

SOURCE = native.source("voxel_host.cpp")
NAMES = ("pn_voxel_f32", "pn_voxel_workspace_bytes", "pn_voxel_launches")
TILE = 1024      # VX_TILE of csrc/voxel_math.h (test_the_tile_is_the_one_the_tests_assume)
LAUNCHES = 7
CELLS = 2 ** 20  # cells -2^20 .. 2^20 - 1 per axis


# ---------------------------------------------------------------------------------------------
# the definition, in numpy and Python integers (shared with tests/test_voxel_gpu.py)
# ---------------------------------------------------------------------------------------------
def voxel_numpy(P, h, origin=None):
    """One cloud by the definition: (owner (n) int32, nvox int, centroid (n,3) fp32, count, first, rep (n) int32); the
    voxel arrays in the first nvox rows, NaN / -1 behind them; nvox -1 / -2: the statuses."""
    P = np.ascontiguousarray(P, np.float32).reshape(-1, 3)
    n = P.shape[0]
    owner, centroid = np.full(n, -1, np.int32), np.full((n, 3), np.nan, np.float32)
    count, first, rep = (np.full(n, -1, np.int32) for _ in range(3))
    h = np.float32(h)
    o = None if origin is None else np.asarray(origin, np.float32).reshape(3)
    status = 0
    if not np.isfinite(P).all():
        status = -1
    elif not (h > 0 and np.isfinite(h)) or (o is not None and not np.isfinite(o).all()):
        status = -2
    if status or n == 0:
        return owner, status, centroid, count, first, rep
    lo, hi = P.min(0), P.max(0)
    o = lo if o is None else o
    cell = np.floor((P.astype(np.float64) - o.astype(np.float64)) / np.float64(h))       # fp64, one rounding each
    if not ((cell >= -CELLS) & (cell < CELLS)).all():
        return owner, -2, centroid, count, first, rep
    members = {}                                                   # cell triple -> indices, in order of first arrival
    for i, c in enumerate(map(tuple, cell.astype(np.int64).tolist())):
        members.setdefault(c, []).append(i)
    ext = max(float(hi[a]) - float(lo[a]) for a in range(3))
    s = 32 - math.frexp(ext)[1] if ext > 0 else 0
    u = [[round(math.ldexp(float(P[i, a]) - float(lo[a]), s)) for a in range(3)] for i in range(n)]     # Python ints
    with np.errstate(over="ignore"):
        for v, m in enumerate(members.values()):
            owner[m] = v
            for a in range(3):
                U = sum(u[i][a] for i in m)
                assert 0 <= U < 2 ** 64
                centroid[v, a] = np.float32(float(lo[a]) + math.ldexp(float(U) / float(len(m)), -s))
            count[v], first[v] = len(m), m[0]
            dx, dy, dz = (P[m, a] - centroid[v, a] for a in range(3))
            d = (dx * dx + dy * dy) + dz * dz
            assert d.dtype == np.float32
            rep[v] = m[int(np.argmin(d))]                         # the first minimum: the lowest index
    return owner, len(members), centroid, count, first, rep


def voxel_numpy_batch(clouds, sizes, origins=None):
    """A ragged batch: (owner (total), nvox (S), centroid (total,3), count, first, rep (total))."""
    out = [voxel_numpy(P, h, None if origins is None else origins[c]) for c, (P, h) in enumerate(zip(clouds, sizes))]
    return tuple(np.asarray([o[1] for o in out], np.int32) if t == 1 else
                 np.concatenate([o[t] for o in out]) for t in range(6))


def cell_map(P, h, origin, result):
    """cell triple -> (centroid bits, count) of a valid result: what a permutation of the points must not change."""
    owner, V, centroid, count = result[:4]
    o = P.min(0) if origin is None else np.asarray(origin, np.float32)
    cell = np.floor((P.astype(np.float64) - o.astype(np.float64)) / np.float64(np.float32(h))).astype(np.int64)
    out = {}
    for i, v in enumerate(owner.tolist()):
        out.setdefault(tuple(cell[i].tolist()), set()).add((centroid[v].tobytes(), int(count[v])))
    assert all(len(x) == 1 for x in out.values()) and len(out) == V
    return out


def check_properties(P, h, origin, result):
    """The exact properties of one valid cloud."""
    owner, V, centroid, count, first, rep = result
    n = P.shape[0]
    assert V >= 1 and count[:V].sum() == n and (count[V:] == -1).all() and (first[V:] == -1).all()
    assert (rep[V:] == -1).all() and np.isnan(centroid[V:]).all() and np.isfinite(centroid[:V]).all()
    assert first[0] == 0 and owner[0] == 0 and (np.diff(first[:V]) > 0).all()
    assert np.array_equal(owner[first[:V]], np.arange(V)) and np.array_equal(owner[rep[:V]], np.arange(V))
    assert np.array_equal(np.bincount(owner, minlength=V), count[:V])
    # every centroid inside the closed box of its cell, widened by one fp32 ulp
    o = (P.min(0) if origin is None else np.asarray(origin, np.float32)).astype(np.float64)
    h = np.float64(np.float32(h))
    cell = np.floor((P[first[:V]].astype(np.float64) - o) / h)
    lo, hi = o + cell * h, o + (cell + 1) * h
    with np.errstate(over="ignore"):
        ulp = np.spacing(np.maximum(np.abs(lo), np.abs(hi)).astype(np.float32)).astype(np.float64)
    c = centroid[:V].astype(np.float64)
    assert ((c >= lo - ulp) & (c <= hi + ulp)).all()


def uniform(n, seed=None):
    return np.random.RandomState(n if seed is None else seed).uniform(-1, 1, (n, 3)).astype(np.float32)


ALONE, BETWEEN, ONE = 1e-5, 0.25, 4.0            # on uniform(-1, 1): every point alone, some hundred voxels, one voxel
SIZES = (1, 2, 3, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)


def cases():
    """name -> (cloud, voxel size, origin or None)."""
    out = {
        # 1 331 points on two tiles, h the spacing and an origin on the lattice: every point lies on a face
        "lattice on its faces": (lattice(11), 0.25, (-0.5, 0.0, 0.25)),
        "lattice, two points per axis": (lattice(11), 0.5, None),
        "copies among random": (copies_among_random(600, 400), 0.1, None),
        "offset, 1e-4 spacing": (offset_cloud(700), 3e-4, None),
        "offset, origin at zero": (offset_cloud(700), 3e-4, (0.0, 0.0, 0.0)),
        "planar": (planar(500), 0.2, None),
        "collinear": (collinear(300), 0.05, (0.3, 0.3, 0.3)),
    }
    for n in SIZES:
        P = uniform(n)
        out["uniform %d, one voxel" % n] = (P, ONE, None)
        out["uniform %d, every point alone" % n] = (P, ALONE, None)      # at 2 049 points: collisions in the table
        out["uniform %d, between" % n] = (P, BETWEEN, None)
        out["uniform %d, negative cells" % n] = (P, BETWEEN, (0.3, 0.3, 0.3))
    return out


def huge():
    return (np.random.RandomState(21).uniform(-1, 1, (50, 3)) * 3e38).astype(np.float32)


# ---------------------------------------------------------------------------------------------
# the host-compiled header
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return native.build_harness(tmp_path_factory.mktemp("vxh"), "vxh", SOURCE)


def host_voxel(lib, batch, sizes, origins=None, cap_mul=2, order=0):
    n = [c.shape[0] for c in batch]
    off = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
    S, total = len(batch), int(off[-1])
    P = np.ascontiguousarray(np.concatenate([c.reshape(-1, 3) for c in batch]), np.float32)
    vox = np.asarray(sizes, np.float32)
    org = None if origins is None else np.ascontiguousarray(origins, np.float32).reshape(S, 3)
    owner, nvox = np.full(total, -9, np.int32), np.full(S, -9, np.int32)
    centroid = np.full((total, 3), -9, np.float32)
    count, first, rep = (np.full(total, -9, np.int32) for _ in range(3))
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    rc = lib.vxh_voxel(p(P), p(off), S, total, p(vox), p(org), cap_mul, order, p(owner), p(nvox), p(centroid), p(count),
                       p(first), p(rep))
    assert rc == LAUNCHES == lib.vxh_launches()
    return owner, nvox, centroid, count, first, rep


def equal(got, want):
    return all(same(np.asarray(g), np.asarray(w, np.asarray(g).dtype)) for g, w in zip(got, want))


def test_the_tile_is_the_one_the_tests_assume(harness):
    assert harness.vxh_tile() == TILE


@pytest.mark.parametrize("name", sorted(cases()))
def test_the_restated_schedule_equals_the_definition(harness, name):
    P, h, origin = cases()[name]
    want = voxel_numpy(P, h, origin)
    for cap_mul, order in ((2, 0), (2, 1), (3, 0), (5, 1)):
        got = host_voxel(harness, [P], [h], None if origin is None else [origin], cap_mul, order)
        assert equal(got, (want[0], [want[1]]) + want[2:]), (name, cap_mul, order)
    check_properties(P, h, origin, want)
    n = P.shape[0]
    if "one voxel" in name:
        assert want[1] == 1 and want[3][0] == n
    if "alone" in name:
        assert want[1] == n and np.array_equal(want[5], np.arange(n)) and (want[3] == 1).all()
    if name == "lattice on its faces":                  # a point on a face belongs to the upper cell: 11^3 voxels
        assert want[1] == n and (want[3] == 1).all()
    if name == "lattice, two points per axis":
        assert want[1] == 6 ** 3 and want[3][0] == 8
    if "negative cells" in name and n > 3:
        assert (np.floor((P.astype(np.float64) - np.float64(np.float32(0.3))) / BETWEEN) < 0).any()


def test_a_permutation_moves_the_numbering_only(harness):
    """The map from the cell to (centroid bits, count) does not see the order of the points; a floating-point sum in
    the order of arrival would."""
    for name in ("uniform 2049, between", "uniform 1025, negative cells", "copies among random",
                 "offset, origin at zero", "lattice, two points per axis"):
        P, h, origin = cases()[name]
        want = cell_map(P, h, origin, voxel_numpy(P, h, origin))
        for seed in (1, 2):
            Q = P[np.random.RandomState(seed).permutation(P.shape[0])]
            ref = voxel_numpy(Q, h, origin)
            assert cell_map(Q, h, origin, ref) == want, name
            got = host_voxel(harness, [Q], [h], None if origin is None else [origin], 2, seed - 1)
            assert equal(got, (ref[0], [ref[1]]) + ref[2:]), name


def test_huge_coordinates_do_not_trap(harness):
    P = huge()
    for h, origin, status in ((1e38, None, None), (2.5e38, (0.0, 0.0, 0.0), None), (1.0, None, -2), (1e-45, None, -2),
                              (3e38, (-3e38, 3e38, 0.0), None)):
        want = voxel_numpy(P, h, origin)
        assert want[1] == status if status else want[1] > 1
        for cap_mul, order in ((2, 0), (3, 1)):
            got = host_voxel(harness, [P], [h], None if origin is None else [origin], cap_mul, order)
            assert equal(got, (want[0], [want[1]]) + want[2:]), (h, origin)


def ragged_batch():
    """clouds, voxel sizes, origins: a tile + 300 points, an empty cloud, a NaN cloud, five points, an inf cloud, a cloud
    whose voxel is too small for it, a lattice; a different size per cloud."""
    nan, inf = uniform(40, 3), uniform(TILE + 7, 4)
    nan[11, 1], inf[TILE + 2, 0] = np.nan, -np.inf
    clouds = [uniform(TILE + 300, 5), np.zeros((0, 3), np.float32), nan, uniform(5, 6), inf, uniform(700, 7) * 250,
              lattice(5)]
    sizes = [0.2, 0.3, 0.1, 0.7, 0.15, 1e-4, 0.5]
    origins = [(0.05, -0.1, 0.3), (0, 0, 0), (0, 0, 0), (-1, -1, -1), (0, 0, 0), (0, 0, 0), (0.25, 0.25, 0.25)]
    return clouds, sizes, origins


def test_a_ragged_batch_with_empty_short_non_finite_and_out_of_range_clouds(harness):
    clouds, sizes, origins = ragged_batch()
    for org in (None, origins):
        want = voxel_numpy_batch(clouds, sizes, org)
        assert want[1][1] == 0 and want[1][2] == -1 and want[1][4] == -1 and want[1][5] == -2
        assert want[1][0] > 100 and want[1][3] >= 1 and want[1][6] >= 8
        for cap_mul, order in ((2, 0), (3, 1)):
            assert equal(host_voxel(harness, clouds, sizes, org, cap_mul, order), want)
        # every cloud alone gives what it gives in the batch
        o = 0
        for c, P in enumerate(clouds):
            alone = host_voxel(harness, [P], [sizes[c]], None if org is None else [org[c]])
            n = P.shape[0]
            assert alone[1][0] == want[1][c]
            assert equal([alone[t] for t in (0, 2, 3, 4, 5)], [want[t][o:o + n] for t in (0, 2, 3, 4, 5)])
            o += n
    # a voxel size that is no positive finite number: -2, after the non-finite check
    for bad in (0.0, -1.0, np.inf, np.nan):
        got = host_voxel(harness, clouds[:4], [0.2, bad, bad, bad])
        assert got[1].tolist()[1:] == [-2, -1, -2]
        assert equal(got, voxel_numpy_batch(clouds[:4], [0.2, bad, bad, bad]))


def test_the_program_checks_itself_and_reads_a_file(harness, tmp_path):
    exe = native.build_program(tmp_path, "voxel_host", SOURCE)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "0 differences" in run.stdout, run.stdout
    P, h = offset_cloud(150), np.float32(2.5e-4)
    path = tmp_path / "cloud.txt"
    path.write_text("%d %.9g\n" % (P.shape[0], h) + "".join("%.9g %.9g %.9g\n" % tuple(p) for p in P))
    run = subprocess.run([exe, str(path)], capture_output=True, text=True, check=True)
    want = voxel_numpy(P, h)
    assert [int(x) for x in run.stdout.split()] == [want[1]] + want[0].tolist() and 1 < want[1] < 150


# ---------------------------------------------------------------------------------------------
# the export and the argument checks, which run before anything touches a GPU
# ---------------------------------------------------------------------------------------------
def load_raw():
    return native.load_raw(NAMES)


@pytest.fixture(scope="module")
def lib():
    return load_raw()


def test_the_entry_points_are_exported_and_bound(lib):
    from parsenet_codebase_amd import _lib
    v, i, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    assert _lib.SIGNATURES["pn_voxel_f32"] == (i, [v, v, i, i, v, v, v, v, v, v, v, v, v, ll, v])
    assert _lib.SIGNATURES["pn_voxel_workspace_bytes"] == (ll, [ll, i])
    assert _lib.SIGNATURES["pn_voxel_launches"] == (i, [])
    assert lib.pn_abi_version() == 23 == _lib.CONSTANTS["PN_ABI_VERSION"]                   # added symbols only
    assert all(hasattr(_lib.load(), n) for n in NAMES)
    assert lib.pn_voxel_launches() == LAUNCHES
    w = lib.pn_voxel_workspace_bytes
    # two table slots per point (key, first, count, three sums), known from (total, S) alone, linear in total
    assert w(1024, 3) >= 2 * 1024 * (8 + 4 + 4 + 24)
    assert w(2048, 3) - w(1024, 3) == w(3072, 3) - w(2048, 3) == w(4096 + 1024, 1) - w(4096, 1) > 0
    assert w(1024, 4) > w(1024, 3)
    assert w(2 * 10 ** 9, 1) > 2 ** 32                                                        # long long, not int
    assert w(2 ** 31, 1) == 0 and w(-1, 1) == 0 and w(10, -1) == 0 and w(2 ** 31 - 1, 1) > 0


ARGS = ("pts", "off", "S", "total", "voxel", "origin", "owner", "nvox", "centroid", "count", "first", "rep", "ws",
        "ws_bytes", "stream")


def raw_call(lib, **over):
    """pn_voxel_f32 with plausible arguments (never dereferenced by a call that is refused), some replaced."""
    a = dict(pts=64, off=64, S=1, total=10, voxel=64, origin=None, owner=64, nvox=64, centroid=None, count=None,
             first=None, rep=None, ws=64, ws_bytes=lib.pn_voxel_workspace_bytes(10, 1), stream=None)
    a.update(over)
    return lib.pn_voxel_f32(*[a[n] for n in ARGS])


def check_invalid_arguments(lib, **real):
    """S < 0, a total that is negative or does not fit the int, a null required pointer, a short workspace:
    PN_ERR_ARG, the message naming the function and the argument; nothing to do: 0."""
    from parsenet_codebase_amd import _lib
    err = _lib.CONSTANTS["PN_ERR_ARG"]
    need = lib.pn_voxel_workspace_bytes(real.get("total", 10), real.get("S", 1))
    for over, word in ((dict(S=-1), b"S=-1"), (dict(total=-1), b"total=-1"), (dict(total=-2 ** 31), b"total="),
                       (dict(pts=None), b"null"), (dict(off=None), b"null"), (dict(voxel=None), b"null"),
                       (dict(owner=None), b"null"), (dict(nvox=None), b"null"), (dict(ws=None), b"null"),
                       (dict(ws_bytes=need - 1), b"workspace"), (dict(ws_bytes=0), b"workspace")):
        assert raw_call(lib, **dict(real, **over)) == err, over
        assert b"pn_voxel_f32" in lib.pn_last_error() and word in lib.pn_last_error(), (over, lib.pn_last_error())
    assert raw_call(lib, **dict(real, nvox=None)) == err                            # the message lists what is required
    assert all(name in lib.pn_last_error() for name in (b"pts", b"off", b"voxel", b"owner", b"nvox", b"ws"))
    assert raw_call(lib, **dict(real, S=0)) == 0
    assert raw_call(lib, **dict(real, total=0)) == 0
    assert raw_call(lib, **dict(real, S=0, pts=None, owner=None, nvox=None, ws=None, ws_bytes=0)) == 0
    assert raw_call(lib, **dict(real, total=0, pts=None, voxel=None, ws=None, ws_bytes=0)) == 0


def test_invalid_arguments_are_refused_before_any_launch(lib):
    """(No GPU is needed to get here: a refused call, and one with nothing to do, launch nothing.)"""
    check_invalid_arguments(lib)


def test_python_argument_checks_need_no_gpu():
    import torch
    from parsenet_codebase_amd import kernels, sampling
    P = torch.zeros(8, 3)
    with pytest.raises(RuntimeError, match="MI355X only"):
        kernels.voxel_ragged(P, torch.tensor([0, 8], dtype=torch.int32), torch.ones(1))
    with pytest.raises(RuntimeError, match="MI355X only"):
        sampling.voxel_downsample(P, 0.1)
    with pytest.raises(RuntimeError, match="MI355X only"):
        sampling.voxel_downsample([P, P], [0.1, 0.2], origin=[[0, 0, 0], [1, 1, 1]], position="point")
    for voxel in (0, -1, float("inf"), float("nan"), True, "a", 1e-60, [0.0], None):
        with pytest.raises(ValueError, match="voxel must be"):
            sampling.voxel_downsample(P, voxel)
    for voxel in ([0.1], [0.1, 0.2, 0.3], np.asarray([0.1, 0.2, 0.3])):
        with pytest.raises(ValueError, match="one size per cloud"):
            sampling.voxel_downsample([P, P], voxel)
    with pytest.raises(ValueError, match="voxel must be"):
        sampling.voxel_downsample([P, P], [0.1, 0.0])
    for origin in ((0, 0), (0, 0, float("nan")), (0, 0, float("inf")), "abc", 1.0, [[0, 0, 0]] * 3, (0, 0, True)):
        with pytest.raises(ValueError, match="origin must be"):
            sampling.voxel_downsample(torch.zeros(2, 8, 3), 0.1, origin=origin)
    for position in ("mean", None, 0, "Centroid"):
        with pytest.raises(ValueError, match="position must be"):
            sampling.voxel_downsample(P, 0.1, position=position)
