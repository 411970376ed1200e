"""The kernels of csrc/edge.hip one by one against fp64 / exact references built on the CPU from their
definitions — on the paths the layer-level oracle tests never take: neighbour lists that do not fit in
registers (k > 128), 2 to 16 points per wave, exact ties of the maximum, transposed-graph lists longer
than one sort (1024 entries), hubs in the second LDS window, more than 64 builder workgroups, targets
nobody names and rows that repeat a neighbour.

What is exact is compared bit for bit (the extreme of y = P[j] + Q[i]: one fp32 addition; its slot; the
transposed graph).  What is summed gets the bound of ANY order of n fp32 additions of exact terms,
|err| <= n * 2^-24 * sum|term|, worked out per element in fp64 — no tolerance here was tuned on a result.
"""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24          # unit roundoff of fp32


def _align256(n):
    return (n + 255) // 256 * 256


# ----------------------------------------------------------------------------------------------------
# A. forward gather-reduce
# ----------------------------------------------------------------------------------------------------
def _fwd_inputs(B, N, k, Cout, seed):
    """PQ, idx (int64), gamma with planted ties of the extreme.

    gamma has both signs, a 0.0 and a -0.0.  Points 3 and 5 (the twins) carry the SAME P row, pushed far to
    the side that wins in every channel (+6 where the channel takes the maximum, -6 where it takes the
    minimum): a row that names both, or one of them twice, ties in every channel.  Other rows repeat a random
    neighbour, which ties in the channels where that neighbour happens to be the extreme."""
    rng = np.random.default_rng(seed)
    PQ = rng.standard_normal((B, N, 2 * Cout)).astype(np.float32)
    gamma = rng.standard_normal(Cout).astype(np.float32)
    gamma[1], gamma[2] = 0.0, -0.0
    side = np.where(gamma >= 0, 6.0, -6.0).astype(np.float32)
    PQ[:, 3, :Cout] = side + 0.25 * PQ[:, 3, :Cout]
    PQ[:, 5, :Cout] = PQ[:, 3, :Cout]
    idx = rng.integers(0, N, (B, N, k))
    if k >= 2:
        # slot pairs: neighbours in one lane, in different row groups of the wave (a row group takes the slots
        # kk % RPI == rg, RPI = 4, 2, 1 rows per step at Cout = 64, 128, >= 256), first against last slot
        pairs = sorted({(0, 1), (0, k - 1), (1, k - 1), (1, min(2, k - 1)), (0, min(4, k - 1)), (k // 2, k - 1),
                        (min(3, k - 1), min(64, k - 1)), (min(1, k - 1), min(130, k - 1))} - {(s, s) for s in range(k)})
        pairs = [(a, b) for a, b in pairs if a < b]
        for r in range(N):
            a, b = pairs[r % len(pairs)]
            kind = (r // len(pairs)) % 4
            if kind == 0:                      # one random neighbour in two slots
                idx[:, r, b] = idx[:, r, a]
            elif kind == 1:                    # a twin in two slots
                idx[:, r, a] = idx[:, r, b] = 3
            elif kind == 2:                    # two different points with identical P rows
                idx[:, r, a], idx[:, r, b] = 5, 3
            # kind 3: the row stays random
    return PQ, idx, gamma


def _ref_fwd(PQ, idx, gamma, groups, per_sample):
    B, N, C2 = PQ.shape
    Cout = C2 // 2
    k = idx.shape[2]
    Cg = Cout // groups
    pos = gamma >= 0
    yext = np.empty((B, N, Cout), np.float32)
    argk = np.empty((B, N, Cout), np.int64)
    S, A = np.empty((B, N, Cout)), np.empty((B, N, Cout))
    g1, a1, g2 = (np.empty((B, groups)) for _ in range(3))
    for b in range(B):
        y = PQ[b, :, :Cout][idx[b]] + PQ[b, :, None, Cout:]          # fp32 + fp32: the kernel's own bits
        assert y.dtype == np.float32
        yext[b] = np.where(pos, y.max(1), y.min(1))
        argk[b] = np.where(pos, y.argmax(1), y.argmin(1))            # numpy: the FIRST slot that attains it
        y = y.astype(np.float64)
        S[b], A[b] = y.sum(1), np.abs(y).sum(1)
        g1[b] = S[b].reshape(N, groups, Cg).sum((0, 2))
        a1[b] = A[b].reshape(N, groups, Cg).sum((0, 2))
        g2[b] = (y * y).sum(1).reshape(N, groups, Cg).sum((0, 2))
    if not per_sample:
        g1, a1, g2 = g1.sum(0, keepdims=True), a1.sum(0, keepdims=True), g2.sum(0, keepdims=True)
    return yext, argk, S, A, g1, a1, g2


def _n_for(ppw):
    # three full workgroups of 4 waves, then one wave of ppw points and one that stops after its first point
    return 3 * (4 * ppw) + ppw + 1


#            Cout   k  ppw  int32 per_sample groups B
FWD_CASES = [(64, 1, None, False, True, 1, 1),
             (64, 2, 2, True, False, 2, 3),
             (64, 63, 4, False, True, 64, 1),
             (64, 64, 8, True, True, 2, 3),
             (64, 65, 16, False, False, 1, 1),
             (64, 127, None, True, True, 2, 1),
             (64, 128, 4, False, False, 64, 3),
             (64, 129, 8, True, True, 1, 1),
             (64, 200, 16, False, True, 2, 3),
             (64, 255, 2, True, False, 2, 1),
             (128, 1, 4, True, False, 1, 3),
             (128, 65, None, False, True, 128, 3),
             (128, 128, 16, True, False, 2, 1),
             (128, 129, 4, False, True, 1, 3),
             (128, 255, 8, True, True, 2, 1),
             (256, 2, 8, False, False, 256, 3),
             (256, 64, 2, True, True, 1, 1),
             (256, 129, 16, False, True, 2, 1),
             (256, 255, 4, True, False, 2, 3),
             (512, 63, 4, False, True, 2, 3),
             (512, 127, None, True, False, 512, 1),
             (512, 200, 2, False, True, 1, 1),
             (512, 255, 8, True, False, 2, 1),
             (40, 1, None, True, True, 2, 1),
             (40, 65, 4, False, False, 1, 3),
             (40, 129, None, True, False, 40, 3),
             (40, 255, None, False, True, 2, 1)]


@pytest.mark.parametrize("Cout,k,ppw,int32,per_sample,groups,B", FWD_CASES)
def test_reduce_fwd_exact_extreme_first_slot_and_bounded_sums(gpu, monkeypatch, Cout, k, ppw, int32, per_sample,
                                                             groups, B):
    from parsenet_codebase_amd import kernels
    if ppw is None:
        monkeypatch.delenv("PN_EC_PPW", raising=False)
    else:
        monkeypatch.setenv("PN_EC_PPW", str(ppw))
    N = _n_for(ppw or 2) if Cout != 40 else 37               # the generic kernel: 16 points per workgroup
    PQ, idx, gamma = _fwd_inputs(B, N, k, Cout, 1000 * Cout + k)
    ti = torch.from_numpy(idx)
    yext, argk, s1, stats = kernels.edgeconv_reduce_fwd(torch.from_numpy(PQ).to(gpu),
                                                        (ti.int() if int32 else ti).to(gpu),
                                                        torch.from_numpy(gamma).to(gpu), groups, per_sample)
    assert argk.dtype == torch.uint8 and stats.dtype == torch.float64
    assert stats.shape == (B if per_sample else 1, groups, 2)
    yext, argk, s1, stats = yext.cpu().numpy(), argk.cpu().numpy(), s1.cpu().numpy(), stats.cpu().numpy()
    r_yext, r_argk, S, A, g1, a1, g2 = _ref_fwd(PQ, idx, gamma, groups, per_sample)
    if k >= 2:   # the planted ties are there: rows whose first extreme slot has a later twin, on both sides
        y0 = PQ[0, :, :Cout][idx[0]] + PQ[0, :, None, Cout:]
        tied = (y0 == r_yext[0][:, None, :]).sum(1) > 1
        assert tied[:, gamma >= 0].any() and tied[:, gamma < 0].any()
    assert np.array_equal(yext, r_yext)
    bad = np.argwhere(argk != r_argk)
    assert bad.size == 0, "argk differs at (b, i, c) = %s: %d, first slot %d" % (
        bad[0], argk[tuple(bad[0])], r_argk[tuple(bad[0])])
    assert np.all(np.abs(s1.astype(np.float64) - S) <= k * U * A)
    assert np.all(np.abs(stats[..., 0] - g1) <= (k * U + 1e-12) * a1)
    assert np.all(np.abs(stats[..., 1] - g2) <= ((k + 1) * U + 1e-12) * g2)


def test_k_256_is_refused_and_nothing_is_written(gpu):
    """argk is uint8: slot 256 would wrap to 0.  The wrapper raises; called through the C ABI with buffers of its
    own, the entry point returns an error and launches nothing."""
    from parsenet_codebase_amd import _lib, kernels
    B, N, k, Cout = 1, 300, 256, 64
    g = torch.Generator().manual_seed(5)
    PQ = torch.randn(B, N, 2 * Cout, generator=g).to(gpu)
    gamma = torch.randn(Cout, generator=g).to(gpu)
    idx = torch.randint(0, N, (B, N, k), generator=g).to(gpu)
    for graph in (idx, idx.int()):
        with pytest.raises(RuntimeError, match="k=256"):
            kernels.edgeconv_reduce_fwd(PQ, graph, gamma, 2, True)
        with pytest.raises(RuntimeError, match="k=256"):
            kernels.edgeconv_csr_build(graph)
    lib = _lib.load()
    yext = torch.full((B, N, Cout), 7.0, device=gpu)
    s1 = torch.full((B, N, Cout), 7.0, device=gpu)
    argk = torch.full((B, N, Cout), 9, dtype=torch.uint8, device=gpu)
    stats = torch.full((B, 2, 2), 7.0, dtype=torch.float64, device=gpu)
    wsz = lib.pn_edgeconv_reduce_workspace(B, N, Cout, 2)
    ws = torch.full((wsz,), 9, dtype=torch.uint8, device=gpu)
    rc = lib.pn_edgeconv_reduce_fwd_f32(_lib.ptr(PQ), _lib.ptr(idx), _lib.ptr(gamma), B, N, k, Cout, 2, 1,
                                        _lib.ptr(yext), _lib.ptr(argk), _lib.ptr(s1), _lib.ptr(stats), _lib.ptr(ws),
                                        wsz, _lib.current_stream(gpu))
    assert rc != 0
    torch.cuda.synchronize()
    assert bool((yext == 7.0).all()) and bool((s1 == 7.0).all()) and bool((argk == 9).all())
    assert bool((stats == 7.0).all()) and bool((ws == 9).all())


# ----------------------------------------------------------------------------------------------------
# B. the transposed graph
# ----------------------------------------------------------------------------------------------------
def _rand_rows(rng, N, k, lo=0):
    return rng.integers(lo, N, (N, k))


def _g_random(rng, item):
    return _rand_rows(rng, 300, 7)


def _g_hub3000(rng, item):
    # a list of (at least) 3000 entries: sorted bucket by bucket; the second item names another hub from fewer rows
    idx = _rand_rows(rng, 3000, 4)
    if item == 0:
        idx[:, 0] = 5
    else:
        idx[:2500, 0] = 2998
    return idx


def _g_cap(rng, item):
    # lists of exactly 1024 (one sort) and 1025 entries (the first length sorted by buckets)
    idx = _rand_rows(rng, 2000, 3, lo=3)
    r0 = 0 if item == 0 else 500
    idx[r0:r0 + 1024, 1] = 1
    idx[r0:r0 + 1025, 2] = 2
    return idx


def _g_deg0(rng, item):
    # two targets in three are named by nobody (0 and 1 among them); the hub is the last point
    N = 1200
    idx = 3 * rng.integers(1, N // 3, (N, 3))
    idx[:, 0] = N - 1
    if item == 1:
        idx[::2, 2] = N - 1
    return idx


def _g_window(N):
    def make(rng, item):
        # hubs on both sides of the boundary between the LDS windows (16384 counters) and at the last point
        hubs = sorted({16383, min(16384, N - 1), N - 1})
        idx = _rand_rows(rng, N, 2)
        rows = np.arange(1100 * len(hubs)) + 37 * item
        idx[rows, item] = np.asarray(hubs)[rows % len(hubs)]
        return idx
    return make


def _g_wg65(rng, item):
    # 66000 points: 65 builder workgroups per item; one hub named by every 50th row, in every workgroup's chunk
    idx = _rand_rows(rng, 66000, 2)
    idx[item::50, 1] = 33000 + item
    return idx


def _g_multiset(rng, item):
    # every entry names one target: a workgroup's bucket holds 9000 * 8 / 64 = 1125 > 1024 entries
    return np.full((9000, 8), 4321 if item == 0 else 0)


GRAPHS = {"random": _g_random, "hub3000": _g_hub3000, "cap1024": _g_cap, "deg0": _g_deg0,
          "win16384": _g_window(16384), "win16385": _g_window(16385), "win20000": _g_window(20000),
          "wg65": _g_wg65, "multiset": _g_multiset}
_graph_cache = {}


def _graph(name):
    """(idx (2,N,k) int64, off (2,N+1), rev (2,N*k)): a graph of two different items and its transposed CSR by a
    stable argsort; computed once and shared, never modified."""
    if name not in _graph_cache:
        rng = np.random.default_rng(sorted(GRAPHS).index(name))
        idx = np.stack([GRAPHS[name](rng, item) for item in range(2)]).astype(np.int64)
        B, N, k = idx.shape
        off = np.zeros((B, N + 1), np.int64)
        rev = np.empty((B, N * k), np.int64)
        for b in range(B):
            flat = idx[b].reshape(-1)
            order = np.argsort(flat, kind="stable")
            rev[b] = ((order // k) << 8) | (order % k)
            off[b, 1:] = np.cumsum(np.bincount(flat, minlength=N))
        for a in (idx, off, rev):
            a.setflags(write=False)
        _graph_cache[name] = (idx, off, rev)
    return _graph_cache[name]


def _decode_csr(ws, B, N, k):
    """off (B,N+1) int32 and rev (B,N*k) uint32 out of the workspace of edgeconv_csr_build (the layout of
    pn_build_rev_csr: degrees, offsets, lists, each aligned to 256 bytes)."""
    o0 = _align256(B * N * 4)
    r0 = o0 + _align256(B * (N + 1) * 4)
    raw = ws[:r0 + B * N * k * 4].cpu().numpy()
    off = raw[o0:o0 + B * (N + 1) * 4].view(np.int32).reshape(B, N + 1)
    rev = raw[r0:r0 + B * N * k * 4].view(np.uint32).reshape(B, N * k)
    return off, rev


def test_graph_fixtures_have_the_lists_the_builder_paths_need():
    # (a property of the fixtures, not of the library: they must keep the lists that take the builder's long paths)
    def deg(name, b, j):
        _, off, _ = _graph(name)
        return int(off[b, j + 1] - off[b, j])
    assert deg("hub3000", 0, 5) >= 3000 and deg("hub3000", 1, 2998) >= 2500
    for b in range(2):
        assert deg("cap1024", b, 1) == 1024 and deg("cap1024", b, 2) == 1025
        assert deg("deg0", b, 0) == 0 and deg("deg0", b, 1) == 0 and deg("deg0", b, 1199) >= 1200
        assert (np.diff(_graph("deg0")[1][b]) == 0).sum() > 700
        for N in (16384, 16385, 20000):
            for j in {16383, min(16384, N - 1), N - 1}:
                assert deg("win%d" % N, b, j) > 1024
        assert deg("wg65", b, 33000 + b) >= 1320
        assert deg("multiset", b, 0 if b else 4321) == 72000


@pytest.mark.parametrize("int32", [False, True])
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_csr_build_equals_the_stable_argsort(gpu, name, int32):
    from parsenet_codebase_amd import kernels
    idx, r_off, r_rev = _graph(name)
    B, N, k = idx.shape
    ti = torch.from_numpy(idx.copy())
    ws = kernels.edgeconv_csr_build((ti.int() if int32 else ti).to(gpu))
    off, rev = _decode_csr(ws, B, N, k)
    assert np.array_equal(off, r_off)
    if name == "multiset":
        # buckets over the sort's capacity are left as filled: every list holds the right entries, in some order
        for b in range(B):
            seg = np.repeat(np.arange(N), np.diff(r_off[b]))
            assert np.array_equal(rev[b][np.lexsort((rev[b], seg))], r_rev[b])
        return
    bad = np.argwhere(rev != r_rev)
    assert bad.size == 0, "%d entries differ, the first at (item, position) %s: 0x%x, expected 0x%x" % (
        len(bad), bad[0], rev[tuple(bad[0])], r_rev[tuple(bad[0])])


# ----------------------------------------------------------------------------------------------------
# C. backward gathers over the transposed graph
# ----------------------------------------------------------------------------------------------------
def _scatter_rows(idx_b, rows_by_slot, N):
    """out[j] = sum over the edges (i, slot) -> j of rows_by_slot(slot)[i], in fp64."""
    out = None
    for s in range(idx_b.shape[1]):
        src = rows_by_slot(s)
        if out is None:
            out = torch.zeros((N,) + tuple(src.shape[1:]), dtype=torch.float64)
        out.index_add_(0, idx_b[:, s], src)
    return out


def _ref_bwd(PQ, idx, t, s1, argk, mean, rstd, c1c2, groups, per_sample, dense):
    """(dPQ, bound) in fp64 from the closed form above pn_edgeconv_bwd_gather_kernel.  A term of the bound is
    every product that is added into the element: r*deg*c1, r*deg*c2*r*P, r*deg*c2*r*mu, r^2*c2*Q[i] per list
    entry, r*t[i] per extreme edge; k*c1, c2*r*s1, c2*r*k*mu and t for dQ."""
    B, N, C2 = PQ.shape
    Cout = C2 // 2
    k = idx.shape[2]
    ch = torch.arange(Cout) // (Cout // groups)
    ref, bound = torch.empty(B, N, C2, dtype=torch.float64), torch.empty(B, N, C2, dtype=torch.float64)
    PQ, t, s1, mean, rstd, c1c2 = (a.double() for a in (PQ, t, s1, mean, rstd, c1c2))
    for b in range(B):
        s = b if per_sample else 0
        mu, r, c1, c2 = mean[s][ch], rstd[s][ch], c1c2[s, :, 0][ch], c1c2[s, :, 1][ch]
        P, Q = PQ[b, :, :Cout], PQ[b, :, Cout:]
        ref[b, :, Cout:] = r * (t[b] - k * c1 - c2 * r * (s1[b] - k * mu))
        bound[b, :, Cout:] = 8 * U * r.abs() * (t[b].abs() + k * c1.abs() + (c2 * r).abs() * (s1[b].abs() + k * mu.abs()))
        deg = torch.bincount(idx[b].reshape(-1), minlength=N).double()[:, None]
        hit = [(argk[b] == slot).double() for slot in range(k)]
        ext = _scatter_rows(idx[b], lambda slot: t[b] * hit[slot], N)
        ext_abs = _scatter_rows(idx[b], lambda slot: t[b].abs() * hit[slot], N)
        dP, A = r * ext, r.abs() * ext_abs
        if dense:
            sq = _scatter_rows(idx[b], lambda slot: Q, N)
            sq_abs = _scatter_rows(idx[b], lambda slot: Q.abs(), N)
            dP = dP - r * deg * (c1 + c2 * r * (P - mu)) - r * r * c2 * sq
            A = A + r.abs() * deg * (c1.abs() + (c2 * r).abs() * (P.abs() + mu.abs())) + r * r * c2.abs() * sq_abs
        ref[b, :, :Cout] = dP
        bound[b, :, :Cout] = (deg + 8) * U * A
    return ref, bound


#            graph     Cout groups per_sample dense int32
BWD_CASES = [("random", 64, 2, True, True, False),
             ("random", 128, 1, False, False, True),
             ("random", 256, 256, True, False, False),
             ("random", 512, 2, False, True, True),
             ("random", 40, 4, True, True, False),
             ("random", 40, 1, False, False, True),
             ("hub3000", 64, 2, False, True, True),
             ("hub3000", 128, 2, True, True, False),
             ("hub3000", 512, 1, True, False, False),
             ("hub3000", 40, 2, False, True, True),
             ("cap1024", 64, 64, True, False, True),
             ("cap1024", 256, 2, False, True, False),
             ("cap1024", 40, 40, True, True, True),
             ("deg0", 64, 1, True, True, False),
             ("deg0", 128, 128, False, False, True),
             ("deg0", 256, 2, True, True, True),
             ("deg0", 512, 2, False, True, False),
             ("deg0", 40, 2, False, False, False),
             ("multiset", 64, 2, False, True, False),
             ("multiset", 128, 2, True, False, True),
             ("multiset", 40, 1, True, True, False)]


@pytest.mark.parametrize("name,Cout,groups,per_sample,dense,int32", BWD_CASES)
def test_edgeconv_bwd_closed_form_on_hub_graphs(gpu, name, Cout, groups, per_sample, dense, int32):
    from parsenet_codebase_amd import kernels
    idx = torch.from_numpy(_graph(name)[0].copy())
    B, N, k = idx.shape
    g = torch.Generator().manual_seed(Cout + N)
    S = B if per_sample else 1
    PQ = torch.randn(B, N, 2 * Cout, generator=g)
    t = torch.randn(B, N, Cout, generator=g)
    s1 = torch.randn(B, N, Cout, generator=g)
    argk = torch.randint(0, k, (B, N, Cout), generator=g).to(torch.uint8)
    mean = torch.randn(S, groups, generator=g)
    rstd = torch.rand(S, groups, generator=g) * 1.5 + 0.5
    c1c2 = torch.randn(S, groups, 2, generator=g)
    ref, bound = _ref_bwd(PQ, idx, t, s1, argk, mean, rstd, c1c2, groups, per_sample, dense)
    gi = (idx.int() if int32 else idx).to(gpu)
    args = [a.to(gpu) for a in (t, s1, argk, mean, rstd, c1c2)]
    here = kernels.edgeconv_bwd(PQ.to(gpu), gi, *args, groups, per_sample, dense)
    pre = kernels.edgeconv_bwd(PQ.to(gpu), gi, *args, groups, per_sample, dense, csr=kernels.edgeconv_csr_build(gi))
    for out in (here, pre):
        err = (out.cpu().double() - ref).abs()
        bad = torch.nonzero(err > bound)
        assert bad.numel() == 0, "%d elements over their bound, the first at (b, j, c) = %s: error %.3e, bound %.3e" % (
            len(bad), bad[0].tolist(), err[tuple(bad[0].tolist())], bound[tuple(bad[0].tolist())])
    if name != "multiset":      # (there the order inside a list, and with it the last bit, is the LDS unit's)
        assert torch.equal(here, pre)


@pytest.mark.parametrize("C", [3, 70])
@pytest.mark.parametrize("name", ["hub3000", "deg0"])
def test_edge_feature_bwd_closed_form_on_hub_graphs(gpu, name, C):
    """gxt[j] = sum_{(i,slot)->j} g[i,slot,:C] + sum_kk (g[j,kk,C:] - g[j,kk,:C]): deg_j additions of list entries,
    k subtractions and k additions of the centre term."""
    from parsenet_codebase_amd import kernels
    idx = torch.from_numpy(_graph(name)[0].copy())
    B, N, k = idx.shape
    gfeat = torch.randn(B, N, k, 2 * C, generator=torch.Generator().manual_seed(C + N))
    out = kernels.edge_feature_bwd(gfeat.to(gpu), idx.to(gpu)).cpu().double()
    g = gfeat.double()
    for b in range(B):
        ref = _scatter_rows(idx[b], lambda slot: g[b, :, slot, :C], N) + (g[b, :, :, C:] - g[b, :, :, :C]).sum(1)
        A = _scatter_rows(idx[b], lambda slot: g[b, :, slot, :C].abs(), N) + g[b].abs().sum(1).reshape(N, 2, C).sum(1)
        deg = torch.bincount(idx[b].reshape(-1), minlength=N).double()[:, None]
        assert bool(((out[b] - ref).abs() <= (deg + 2 * k) * U * A).all())


# ----------------------------------------------------------------------------------------------------
# D. the whole layer at the new corners, against the torch oracle
# ----------------------------------------------------------------------------------------------------
def _rel(a, b):
    a = a.detach().cpu().double()
    b = b.detach().cpu().double()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


@pytest.mark.parametrize("kind,B,C,Cout,N,k,ppw,int32,hub", [
    ("gn", 1, 16, 64, 150, 130, None, False, False),      # neighbour list read from memory
    ("gn", 2, 6, 64, 200, 10, 8, True, True),            # eight points per wave, int32 graph, a hub
    ("bn", 2, 64, 128, 1500, 3, None, False, True),      # a list of 1500 entries
])
def test_edge_conv_layer_at_the_new_corners(gpu, monkeypatch, kind, B, C, Cout, N, k, ppw, int32, hub):
    from oracle import ref_torch as R
    from parsenet_codebase_amd import graph
    if ppw is None:
        monkeypatch.delenv("PN_EC_PPW", raising=False)
    else:
        monkeypatch.setenv("PN_EC_PPW", str(ppw))
    with torch.random.fork_rng(devices=[]):     # (the global generator is left as it was found for the tests that follow)
        torch.manual_seed(N + Cout)
        x = torch.randn(B, C, N)
        g = torch.Generator().manual_seed(2)
        idx = torch.stack([torch.stack([torch.randperm(N, generator=g)[:k] for _ in range(N)]) for _ in range(B)])
        idx[:, :, 0] = 7 if hub else torch.arange(N)
        conv = torch.nn.Conv2d(2 * C, Cout, 1, bias=False)
        norm = torch.nn.GroupNorm(2, Cout) if kind == "gn" else torch.nn.BatchNorm2d(Cout)
        with torch.no_grad():
            norm.weight.copy_(torch.randn(Cout))
            norm.bias.copy_(torch.randn(Cout) * 0.3)
        wout = torch.randn(B, Cout, N)
    conv_g, norm_g = copy.deepcopy(conv).to(gpu), copy.deepcopy(norm).to(gpu)

    xr = x.clone().requires_grad_(True)
    yr = R.edge_conv(xr, idx, conv, norm)
    (yr * wout).sum().backward()

    xg = x.to(gpu).requires_grad_(True)
    yg = graph.edge_conv_norm_max(xg, (idx.int() if int32 else idx).to(gpu), conv_g.weight, norm_g)
    (yg * wout.to(gpu)).sum().backward()

    assert _rel(yg, yr) < 1e-5
    assert _rel(xg.grad, xr.grad) < 2e-5
    assert _rel(conv_g.weight.grad, conv.weight.grad) < 2e-5
    assert _rel(norm_g.weight.grad, norm.weight.grad) < 2e-5
    assert _rel(norm_g.bias.grad, norm.bias.grad) < 2e-5
    if kind == "bn":
        assert _rel(norm_g.running_mean, norm.running_mean) < 1e-5
        assert _rel(norm_g.running_var, norm.running_var) < 1e-5
        assert int(norm_g.num_batches_tracked) == int(norm.num_batches_tracked)
