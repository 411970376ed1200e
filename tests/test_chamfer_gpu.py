"""Parity of the HIP Chamfer nearest-neighbour kernel against the C oracle (bit-exact
minima and arg-mins) at sizes the oracle finishes in seconds, plus size-independent
properties at the 10k x 10k size of BASELINE.json."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(params=["scalar", "mfma", "auto"], autouse=True)
def chamfer_path(request, monkeypatch):
    """Every test of this file on both kernels — PN_CHAMFER_MFMA=0: the scalar kernel, =1: the matrix-core
    pre-filter with the exact decision (round 6), whatever the size — and on the library's own choice."""
    if request.param == "auto":
        monkeypatch.delenv("PN_CHAMFER_MFMA", raising=False)
    else:
        monkeypatch.setenv("PN_CHAMFER_MFMA", "1" if request.param == "mfma" else "0")
    return request.param


def _run(a, b, gpu):
    from parsenet_codebase_amd import kernels
    ta = torch.from_numpy(a).to(gpu)
    tb = torch.from_numpy(b).to(gpu)
    return [t.cpu().numpy() for t in kernels.chamfer_nn(ta, tb)]


# the last six: min(Na, Nb) on both sides of the matrix-core kernel's wave-count thresholds (4, 16 and 64 candidate
# tiles of 32: 96|97, 480|481, 2016|2017), the other cloud no multiple of 32
@pytest.mark.parametrize("B,Na,Nb", [(1, 1, 1), (1, 7, 300), (3, 257, 129), (32, 1600, 700),
                                     (1, 10000, 3001), (2, 900, 5000),
                                     (2, 96, 333), (1, 333, 97), (1, 717, 480), (2, 481, 717),
                                     (1, 2016, 2333), (1, 2333, 2017)])
def test_bit_exact_vs_oracle(gpu, B, Na, Nb):
    from oracle import cbind
    rng = np.random.RandomState(B * 1000 + Na + Nb)
    a = rng.uniform(-0.5, 0.5, (B, Na, 3)).astype(np.float32)
    b = rng.uniform(-0.5, 0.5, (B, Nb, 3)).astype(np.float32)
    minA, argA, minB, argB = _run(a, b, gpu)
    oA, oiA = cbind.chamfer_nn(a, b)
    oB, oiB = cbind.chamfer_nn(b, a)
    assert np.array_equal(argA, oiA) and np.array_equal(argB, oiB)
    assert np.array_equal(minA.view(np.uint32), oA.view(np.uint32))
    assert np.array_equal(minB.view(np.uint32), oB.view(np.uint32))


# A block of the scalar kernel owns 128 Q queries, row r of lane t is query 128 r + t of the block: sizes one below
# and one above a block of Q = 1 (128) and of Q = 4 (512), two full Q = 4 blocks plus one row; Nb = 255 / 257 on both
# sides of the change from one candidate range to split ranges merged by the 64-bit atomicMin, Nb = 65 / 513 with a
# partial last group after a range aligned to 64.  (The indirect parameter replaces the file's three paths by the
# scalar kernel alone: PN_CHAMFER_Q means nothing to the others.)
@pytest.mark.parametrize("chamfer_path", ["scalar"], indirect=True)
@pytest.mark.parametrize("Q", ["1", "2", "4"])
@pytest.mark.parametrize("B,Na,Nb", [(1, 1, 1), (1, 127, 9), (2, 129, 65), (1, 511, 257), (3, 513, 255),
                                     (1, 1025, 513)])
def test_queries_per_lane_bit_exact_vs_oracle(gpu, monkeypatch, chamfer_path, Q, B, Na, Nb):
    from oracle import cbind
    monkeypatch.setenv("PN_CHAMFER_Q", Q)
    rng = np.random.RandomState(B * 1000 + Na + Nb)
    a = rng.uniform(-0.5, 0.5, (B, Na, 3)).astype(np.float32)
    b = rng.uniform(-0.5, 0.5, (B, Nb, 3)).astype(np.float32)
    minA, argA, minB, argB = _run(a, b, gpu)
    oA, oiA = cbind.chamfer_nn(a, b)
    oB, oiB = cbind.chamfer_nn(b, a)
    assert np.array_equal(argA, oiA) and np.array_equal(argB, oiB)
    assert np.array_equal(minA.view(np.uint32), oA.view(np.uint32))
    assert np.array_equal(minB.view(np.uint32), oB.view(np.uint32))


@pytest.mark.parametrize("side_a,side_b", [(True, False), (False, True)])
@pytest.mark.parametrize("B,Na,Nb", [(2, 257, 129), (1, 700, 1600)])
def test_one_sided_search_bit_exact_vs_oracle(gpu, B, Na, Nb, side_a, side_b):
    """One side requested: the other one is None (on the matrix-core kernel side B alone takes the first slot of the
    launch and sizes grid and waves by itself)."""
    from oracle import cbind
    from parsenet_codebase_amd import kernels
    rng = np.random.RandomState(B * 1000 + Na + Nb)
    a = rng.uniform(-0.5, 0.5, (B, Na, 3)).astype(np.float32)
    b = rng.uniform(-0.5, 0.5, (B, Nb, 3)).astype(np.float32)
    minA, argA, minB, argB = kernels.chamfer_nn(torch.from_numpy(a).to(gpu), torch.from_numpy(b).to(gpu),
                                                side_a, side_b)
    if side_a:
        assert minB is None and argB is None
        got_min, got_arg = minA.cpu().numpy(), argA.cpu().numpy()
        o, oi = cbind.chamfer_nn(a, b)
    else:
        assert minA is None and argA is None
        got_min, got_arg = minB.cpu().numpy(), argB.cpu().numpy()
        o, oi = cbind.chamfer_nn(b, a)
    assert np.array_equal(got_arg, oi)
    assert np.array_equal(got_min.view(np.uint32), o.view(np.uint32))


def _scalar_chunk(B, Nq, Nc, Q):
    """The candidates per split range of the scalar kernel, by the documented rule (chamfer_one_side): 4096 workgroups
    wanted, never a range below 256 candidates, the range rounded up to a multiple of 64."""
    cdiv = lambda x, y: -(-x // y)   # noqa: E731
    qblocks = cdiv(Nq, 128 * Q)
    splits = max(1, min(cdiv(4096, qblocks * B), cdiv(Nc, 256)))
    return cdiv(cdiv(Nc, splits), 64) * 64


# Nc = 1003 next to the 1000: 1000 is a multiple of 8, so only at 1003 (3 past a group of 8, 11 past a tile of 32)
# does the pair (Nc - 2, Nc - 1) lie in the scalar kernel's partial last group.
@pytest.mark.parametrize("chamfer_path,Q", [("scalar", None), ("scalar", "4"), ("mfma", None)],
                         indirect=["chamfer_path"])
@pytest.mark.parametrize("Nc", [1000, 1003])
def test_ties_at_the_seams_resolve_to_the_first_index(gpu, monkeypatch, chamfer_path, Q, Nc):
    """A true tie (coordinates are multiples of 1/64 in [-2, 2]: every difference, square and sum is exact in fp32)
    between exactly two candidates j1 < j2, every other candidate strictly farther, across each place where "the first
    index wins" is decided by other code: inside a group of 8, the group boundary, a tile boundary of the matrix-core
    kernel, the 64-aligned boundary, the boundary of two split ranges (the packed atomicMin), rows 3 | 4 of a tile
    (the two half-waves), and the last two candidates (partial last group, padded rows of the last tile)."""
    from oracle import cbind
    from parsenet_codebase_amd import kernels
    if Q is not None:
        monkeypatch.setenv("PN_CHAMFER_Q", Q)
    Na = 70   # two query tiles of the matrix-core kernel, the second partial
    # the split boundary: computed from the documented rule for THESE sizes (B = 1, 70 queries, Q = 1 or 4: one
    # query block either way) — 256, four ranges
    chunk = _scalar_chunk(1, Na, Nc, int(Q or 1))
    assert chunk < Nc - 2 and chunk % 64 == 0
    pairs = [(0, 1), (7, 8), (31, 32), (63, 64), (chunk - 1, chunk), (Nc - 2, Nc - 1), (32 * 5 + 3, 32 * 5 + 4)]
    queries = [0, 5, 31, 32, 40, 64, 69]   # one query per pair, in both query tiles
    rng = np.random.RandomState(Nc)
    # integer grid coordinates (units of 1/64), candidates and queries all distinct
    cells = rng.randint(0, 255 ** 3, Na + Nc)
    assert len(np.unique(cells)) == Na + Nc
    grid = np.stack([cells % 255, (cells // 255) % 255, cells // (255 * 255)], 1).astype(np.int64) - 127
    qi, ci = grid[:Na].copy(), grid[Na:].copy()
    for i, (j1, j2) in zip(queries, pairs):
        ci[j1] = qi[i] + [1, 0, 0]      # both at squared distance 2^-12
        ci[j2] = qi[i] + [0, -1, 0]
    d_int = ((qi[:, None, :] - ci[None, :, :]) ** 2).sum(2)
    for i, (j1, j2) in zip(queries, pairs):
        assert d_int[i, j1] == d_int[i, j2] == 1 and (np.delete(d_int[i], [j1, j2]) > 1).all()
    a = (qi / 64.0).astype(np.float32)[None]
    b = (ci / 64.0).astype(np.float32)[None]
    assert np.abs(a).max() <= 2 and np.abs(b).max() <= 2
    ta, tb = torch.from_numpy(a).to(gpu), torch.from_numpy(b).to(gpu)
    oA, oiA = cbind.chamfer_nn(a, b)
    oB, oiB = cbind.chamfer_nn(b, a)
    # both sides in one call, then side A alone: the matrix-core kernel takes its wave count from the smaller cloud
    # (70: one wave) when both sides run and from the candidates (32 tiles: four waves, tiles interleaved) otherwise
    for side_b in (True, False):
        minA, argA, minB, argB = kernels.chamfer_nn(ta, tb, True, side_b)
        minA, argA = minA.cpu().numpy(), argA.cpu().numpy()
        for i, (j1, j2) in zip(queries, pairs):
            assert argA[0, i] == j1, (i, j1, j2, int(argA[0, i]))
            assert minA[0, i].view(np.uint32) == np.float32(2.0 ** -12).view(np.uint32)
        assert np.array_equal(argA, oiA)
        assert np.array_equal(minA.view(np.uint32), oA.view(np.uint32))
        if side_b:
            assert np.array_equal(argB.cpu().numpy(), oiB)
            assert np.array_equal(minB.cpu().numpy().view(np.uint32), oB.view(np.uint32))


def test_ties_resolve_to_smallest_index(gpu):
    a = np.zeros((1, 5, 3), np.float32)
    b = np.zeros((1, 4000, 3), np.float32)
    b[0, :, 0] = 1.0
    minA, argA, minB, argB = _run(a, b, gpu)
    assert (argA == 0).all() and (argB == 0).all()
    assert np.allclose(minA, 1.0)


def test_full_size_properties(gpu):
    """10k x 10k (test.py:157-160 size): Chamfer(P,P)=0 with identity arg-min, and a
    permuted copy recovers the permutation."""
    rng = np.random.RandomState(7)
    p = rng.uniform(-0.5, 0.5, (1, 10000, 3)).astype(np.float32)
    perm = rng.permutation(10000)
    q = p[:, perm]
    minA, argA, minB, argB = _run(p, q, gpu)
    assert (minA == 0).all() and (minB == 0).all()
    assert np.array_equal(argB[0], perm)
    assert np.array_equal(perm[argA[0]], np.arange(10000))


@pytest.mark.parametrize("scale,offset", [(1.0, 0.0), (40.0, 0.0), (1.0, 300.0), (1e-3, 0.0), (1.0, -2.5)])
def test_prefilter_bound_holds_far_from_the_origin_and_on_clumps(gpu, scale, offset):
    """The certified bound of the matrix-core pre-filter scales with |q||c|: clouds far from the origin (where the
    norms dwarf the distances and almost every candidate passes the filter), tiny and large extents, tight clumps
    and exact duplicates — minima and arg-mins stay bit-identical to the oracle's."""
    from oracle import cbind
    rng = np.random.RandomState(17)
    a = rng.uniform(-0.5, 0.5, (2, 1500, 3)).astype(np.float32)
    b = rng.uniform(-0.5, 0.5, (2, 2100, 3)).astype(np.float32)
    b[:, 1000:1400] = b[:, 600:1000] + rng.normal(0, 1e-5, (2, 400, 3)).astype(np.float32)     # clumps
    b[:, 1400:1500] = b[:, 100:200]                                                            # exact duplicates
    a[:, :100] = b[:, 1400:1500]                                                               # distance 0, ties
    a = (a * scale + offset).astype(np.float32)
    b = (b * scale + offset).astype(np.float32)
    minA, argA, minB, argB = _run(a, b, gpu)
    oA, oiA = cbind.chamfer_nn(a, b)
    oB, oiB = cbind.chamfer_nn(b, a)
    assert np.array_equal(argA, oiA) and np.array_equal(argB, oiB)
    assert np.array_equal(minA.view(np.uint32), oA.view(np.uint32))
    assert np.array_equal(minB.view(np.uint32), oB.view(np.uint32))


def test_non_finite_coordinates_give_the_empty_key_on_both_kernels(gpu):
    """A query with a NaN / inf coordinate has no finite distance: both kernels leave the "empty" pattern; a
    non-finite CANDIDATE never wins."""
    rng = np.random.RandomState(3)
    a = rng.uniform(-0.5, 0.5, (1, 300, 3)).astype(np.float32)
    b = rng.uniform(-0.5, 0.5, (1, 400, 3)).astype(np.float32)
    a[0, 5, 1] = np.nan
    a[0, 9, 0] = np.inf
    b[0, 17, 2] = np.nan
    minA, argA, minB, argB = _run(a, b, gpu)
    assert argA[0, 5] == 0xffffffff and argA[0, 9] == 0xffffffff
    ok = np.ones(300, bool)
    ok[[5, 9]] = False
    assert (argA[0, ok] != 17).all() and np.isfinite(minA[0, ok]).all()
    d = ((a[0, ok, None, :] - b[0, None, :, :]) ** 2)
    d = (d[..., 0] + d[..., 1]) + d[..., 2]
    d[:, 17] = np.inf
    assert np.array_equal(argA[0, ok], d.argmin(1))
