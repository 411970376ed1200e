"""GPU: the kernels of csrc/fitbatch.hip around the arithmetic that tests/test_fit_math_host.py holds on the CPU —
table indirection (seg_shape / seg_row), chunking over FB_CH, the LDS tiles of FB_TILE, the block reductions, the
strided weight indexing, the status words and the cone's second pass — against the fp64 oracle on every segment's
own slice; the B-spline evaluation kernels off the square grid; pn_sym3_eig_f64 (csrc/fit.hip).

Bars: those of test_fitting_batch_gpu.py::test_primitive_kernels_against_the_oracle per kind and quantity.  One
case is wider, by the reference's own float32 noise: the cone on its angle clamp (CLAMPED_CONE_BARS in
tests/test_fit_math_host.py).  Ground-truth points come from make_gt there (scattered by 0.02), which keeps the
by-design fp32 rounding of the residual below the ordinary distance bar down to a single point."""
import numpy as np
import pytest
import torch

from tests.test_fit_math_host import (CLAMPED_CONE_BARS, CONE_THETA_MAX, EPS32, KINDS, align_sign, clamped_cone_segment,
                                      make_gt, make_segment, null_cone_segment, oracle, sparse_weights)

pytestmark = pytest.mark.gpu
EPS = np.float32(EPS32)
KIND_NAMES = ["plane", "sphere", "cylinder", "cone"]
JUNK = 1e30          # what the off-stride rows of P and Nrm hold where no ground-truth point sits


def _i32(gpu, a):
    return torch.tensor(np.asarray(a), dtype=torch.int32, device=gpu)


def _w_eff(w_stored):
    """The weight the kernels see: the stored fp32 membership plus eps, added in fp32."""
    return (w_stored.astype(np.float32) + EPS).astype(np.float32)


class Launch:
    """One launch of the five stages over a table of segments.  clouds[b] = (P (n,3), Nrm (n,3)) are the strided
    points of shape b; segs = [dict(kind, shape, row, ws (n,) stored memberships, gt (m,3))]; the weights the kernels
    see are left in seg["w"].  Everything the kernels must not read holds junk: off-stride points / normals (1e30),
    off-stride weights and unused rows (random)."""

    def __init__(self, gpu, clouds, segs, N, stride, Cp, sqrt_flag=False, order=None, coeffs=None):
        from parsenet_codebase_amd import kernels as K
        from parsenet_codebase_amd.fitting_batch import _PrimitiveFitLoss
        torch.cuda.set_device(gpu)
        B, n = len(clouds), -(-N // stride)
        rng = np.random.RandomState(1234)
        P = np.full((B, N, 3), JUNK, np.float32)
        Nn = np.full((B, N, 3), -JUNK, np.float32)
        W = rng.rand(B, Cp, N).astype(np.float32)
        free = [[i for i in range(N) if i % stride] for _ in range(B)]     # off-stride slots left in each shape
        for b, (p, nn) in enumerate(clouds):
            assert p.shape == (n, 3) and nn.shape == (n, 3)
            P[b, ::stride], Nn[b, ::stride] = p, nn
        gt_idx = []
        for s in segs:
            b, m = s["shape"], s["gt"].shape[0]
            W[b, s["row"], ::stride] = s["ws"]
            s["w"] = _w_eff(s["ws"])
            idx = np.array(free[b][:m], dtype=np.int64)
            assert idx.size == m, "not enough off-stride slots"
            del free[b][:m]
            P[b, idx] = s["gt"]
            gt_idx.append(idx)
        assert len({(s["shape"], s["row"]) for s in segs}) == len(segs)      # the product's contract
        order = list(range(len(segs))) if order is None else list(order)
        self.order, self.segs, self.n, self.stride = order, segs, n, stride
        counts = [gt_idx[i].size for i in order]
        cat = np.concatenate([gt_idx[i] for i in order]) if sum(counts) else np.zeros(0, np.int64)
        self.tab = {"shape": _i32(gpu, [segs[i]["shape"] for i in order]),
                    "row": _i32(gpu, [segs[i]["row"] for i in order]),
                    "type": _i32(gpu, [KINDS[segs[i]["kind"]] for i in order]),
                    "rows": _i32(gpu, [n] * len(order)),
                    "gt_off": _i32(gpu, np.concatenate([[0], np.cumsum(counts)])),
                    "gt_idx": _i32(gpu, cat)}
        self.W_host = W
        Pg, Ng = torch.from_numpy(P).to(gpu), torch.from_numpy(Nn).to(gpu)
        Wg = torch.from_numpy(W).to(gpu).requires_grad_(True)
        dist, params, status = _PrimitiveFitLoss.apply(Wg, Pg, Ng, self.tab, stride, sqrt_flag)
        coeffs = np.ones(len(segs)) if coeffs is None else np.asarray(coeffs, dtype=np.float64)
        self.coeffs = coeffs
        c = torch.tensor(coeffs[order], dtype=torch.float32, device=gpu)
        (dist * c).sum().backward()
        # the stages once more through the wrappers, for what the autograd function keeps to itself
        tab = self.tab
        partial = K.weighted_moments(Pg, Ng, Wg.detach(), tab["shape"], tab["row"], stride, EPS32)
        p2, jac, st2 = K.primitive_fit(partial, tab["type"], tab["rows"])
        self.fit_status = st2.cpu().numpy().copy()
        cd = K.cone_angle(Pg, Wg.detach(), tab["shape"], tab["row"], tab["type"], st2, p2, jac, stride, EPS32)
        inv = np.argsort(order)                       # results indexed like segs, whatever the launch order
        self.partial = partial.cpu().numpy()[inv]
        self.jac = jac.cpu().numpy()[inv]
        self.cone_direct = cd.cpu().numpy()[inv]
        self.dist = dist.detach().cpu().numpy()[inv]
        self.params = params.cpu().numpy()[inv]
        self.status = status.cpu().numpy()[inv]
        self.fit_status = self.fit_status[inv]
        self.grad = Wg.grad.cpu().numpy()
        assert np.array_equal(p2.cpu().numpy()[inv], self.params, equal_nan=True)

    def seg_grad(self, i):
        s = self.segs[i]
        return self.grad[s["shape"], s["row"], ::self.stride]

    def check_untouched_gradient(self):
        """Exactly zero off the strided columns and in rows no segment uses (pn_wmom_bwd_kernel writes the entries
        (shape, row, stride * j) of its segments and nothing else; the wrapper hands it zeros)."""
        g = self.grad.copy()
        for s in self.segs:
            g[s["shape"], s["row"], ::self.stride] = 0
        assert not g.any()


def check_segment(L, i, clouds, sqrt=False, dist_tol=5e-6, grad_tol=1e-4, label=""):
    """Segment i of launch L against the fp64 oracle on its own slice, at the bars of
    test_primitive_kernels_against_the_oracle."""
    s = L.segs[i]
    kind = s["kind"]
    p, nn = clouds[s["shape"]]
    ref_p, ref_d, ref_g = oracle(kind, p, nn, s["w"], s["gt"], torch.float64, sqrt=sqrt)
    assert np.isfinite(ref_p).all() and np.isfinite(ref_d) and np.isfinite(ref_g).all(), (label, kind, "oracle")
    ref_g = ref_g * L.coeffs[i]
    assert L.status[i] == 0, (label, kind, L.status[i])
    mine = align_sign(kind, L.params[i, :len(ref_p)], ref_p)
    g = L.seg_grad(i)
    scale = np.abs(ref_g).max()
    perr = np.abs(mine - ref_p).max()
    derr, gerr = abs(float(L.dist[i]) - ref_d) / abs(ref_d), np.abs(g - ref_g).max() / scale
    print("%s seg %d %-8s n=%d gt=%d: params %.1e dist %.3e rel %.1e grad rel %.1e ridge %.0e" % (
        label, i, kind, L.n, s["gt"].shape[0], perr, ref_d, derr, gerr, L.params[i, 15]))
    if kind == "cylinder":
        assert L.params[i, 15] > 0                                         # the ridge is in use
        assert np.abs(mine[:3] - ref_p[:3]).max() < 1e-7 and abs(mine[6] - ref_p[6]) < 1e-5 * ref_p[6]
        assert derr < 1e-4
        assert gerr < 1e-3
        return
    tol = 2e-6 if kind == "cone" else 1e-9
    assert perr < tol * max(1.0, np.abs(ref_p).max()), (label, kind, mine, ref_p)
    assert derr < dist_tol, (label, kind, derr)
    assert gerr < grad_tol, (label, kind, gerr)


def _one_per_shape(segments, row=1):
    """(kind, P, Nrm, w, gt) tuples -> clouds and a table with one segment per shape, all in ``row``."""
    clouds = [(p, nn) for _, p, nn, _, _ in segments]
    segs = [dict(kind=k, shape=b, row=row, ws=(w - EPS).astype(np.float32), gt=gt)
            for b, (k, _, _, w, gt) in enumerate(segments)]
    return clouds, segs


# ---- a. table layout ----------------------------------------------------------------------------------------
def _table_case():
    N, stride, Cp = 1199, 4, 5                 # N % stride != 0; n = 300
    n = -(-N // stride)
    seg_shape = [2, 0, 1, 0, 2, 0, 2, 0, 2]    # not sorted; shape 1 hosts a single segment
    seg_row = [1, 3, 2, 0, 4, 4, 0, 1, 2]      # distinct (shape, row) pairs over rows 0..4
    seg_kind = ["cone", "plane", "cone", "sphere", "cylinder", "cylinder", "sphere", "cone", "plane"]
    gt_count = [257, 600, 600, 63, 257, 1, 63, 63, 257]
    members = {b: [i for i in range(9) if seg_shape[i] == b] for b in range(3)}
    clouds, owner = [], {}
    for b in range(3):
        # the cloud of a shape is the union of its segments' primitives, point j belonging to segment j % m
        m = len(members[b])
        parts = [make_segment(seg_kind[i], 100 + i, n=n) for i in members[b]]
        own = np.arange(n) % m
        clouds.append((np.stack([parts[own[j]][0][j] for j in range(n)]),
                       np.stack([parts[own[j]][1][j] for j in range(n)])))
        for k, i in enumerate(members[b]):
            owner[i] = (own == k, parts[k][2])
    segs = []
    rng = np.random.RandomState(77)
    for i in range(9):
        mine, w_own = owner[i]
        # soft memberships: the segment's own weights on its points, a few percent on the others'
        w = np.where(mine, w_own - EPS, 0.05 * rng.rand(n)).astype(np.float32)
        p, nn = clouds[seg_shape[i]]
        own_idx = np.nonzero(mine)[0]
        if gt_count[i] == 1:     # a single point, well off the surface (see make_gt)
            gt = (p[own_idx[:1]] + 0.1 * nn[own_idx[:1]]).astype(np.float32)
        else:
            gt = make_gt(p[own_idx], gt_count[i], 200 + i)
        segs.append(dict(kind=seg_kind[i], shape=seg_shape[i], row=seg_row[i], ws=w, gt=gt))
    coeffs = 0.5 + np.arange(9) * 0.37
    return N, stride, Cp, clouds, segs, coeffs


def test_table_layout(gpu):
    """Nine segments of three shapes in one launch, shapes out of order, five weight rows, junk everywhere the
    kernels must not look; every segment against the oracle on its own slice with its own upstream gradient."""
    N, stride, Cp, clouds, segs, coeffs = _table_case()
    L = Launch(gpu, clouds, segs, N, stride, Cp, coeffs=coeffs)
    assert sorted({s["kind"] for s in segs}) == sorted(KIND_NAMES)
    for i in range(len(segs)):
        check_segment(L, i, clouds, label="table")
    L.check_untouched_gradient()
    # the same table with its segments permuted: bit-identical per-segment results
    perm = [4, 8, 0, 6, 2, 7, 1, 5, 3]
    Lp = Launch(gpu, clouds, segs, N, stride, Cp, coeffs=coeffs, order=perm)
    assert Lp.tab["shape"].cpu().tolist() != L.tab["shape"].cpu().tolist()
    for name in ("dist", "params", "status", "cone_direct", "partial", "jac", "grad"):
        assert np.array_equal(getattr(L, name), getattr(Lp, name)), name


# ---- b. sizes that cross the kernels' seams --------------------------------------------------------------
SEAMS = [(4117, 4), (1027, 4), (2060, 2), (20, 4), (9, 4)]


@pytest.mark.parametrize("N,stride", SEAMS)
def test_sizes_across_the_seams(gpu, N, stride):
    """n = 1030: an LDS tile of 256 plus one of 2 in each chunk; n = 257: chunks of 65, 65, 65, 62 and a backward
    grid of two blocks, the second with one live thread; stride 2; n = 5; n = 3 < FB_CH (the last chunk is empty).
    The CPU oracle is finite for all four kinds at every one of these sizes, n = 3 included (asserted in
    check_segment): no kind is left out."""
    n = -(-N // stride)
    m = min(257, N - n)            # every off-stride slot at the two tiny sizes (6 and 15 points)
    segments = []
    for k, kind in enumerate(KIND_NAMES):
        p, nn, w, _ = make_segment(kind, 20 + k, n=n)
        # few ground-truth points: further off the surface, see make_gt
        segments.append((kind, p, nn, w, make_gt(p, m, 7, sigma=0.02 if m >= 63 else 0.05)))
    clouds, segs = _one_per_shape(segments)
    L = Launch(gpu, clouds, segs, N, stride, 2, coeffs=[1.0, -2.0, 0.5, 3.0])
    for i in range(4):
        check_segment(L, i, clouds, label="N=%d/%d" % (N, stride))
    L.check_untouched_gradient()
    if n != 1030:
        return
    # the moment pass by itself: the chunk sums against the monomial definition of the file header in fp64.
    # Every term is below 1 in magnitude (coordinates of a normalised shape, unit normals, w <= 1 + eps), so a sum
    # of n terms in any order is within n * n * 2^-53.
    assert L.partial.shape == (4, 4, 64)
    for i in range(4):
        p, nn = clouds[i]
        z = np.concatenate([np.ones((n, 1)), p.astype(np.float64), nn.astype(np.float64)], 1)
        w = segs[i]["w"].astype(np.float64)
        ref = np.array([(w ** e * z[:, a] * z[:, b] * z[:, c]).sum() for e, a, b, c in MONOMIALS])
        got = L.partial[i].sum(0)
        err = np.abs(got[:60] - ref).max()
        print("moments seg %d: max abs err %.2e (bar %.2e)" % (i, err, n * n * 2.0 ** -53))
        assert err <= n * n * 2.0 ** -53
        assert not got[60:].any()


def _monomials():
    """The moment table of csrc/fit_math.h restated: moment m = sum_i w_i^e z_i[a] z_i[b] z_i[c] over
    z = [1, px, py, pz, nx, ny, nz]."""
    P3, N3 = (1, 2, 3), (4, 5, 6)
    sym = [(a, b) for a in range(3) for b in range(a, 3)]                     # xx xy xz yy yz zz
    t = []
    for e in (1, 2):
        t += [(e, 0, 0, 0)] + [(e, a, 0, 0) for a in P3] + [(e, a, 0, 0) for a in N3]
        t += [(e, P3[a], P3[b], 0) for a, b in sym]
        if e == 2:
            t += [(e, N3[a], N3[b], 0) for a, b in sym]
            t += [(e, N3[a], N3[b], P3[b]) for a in range(3) for b in range(3)]
    t += [(3, P3[a], P3[b], 0) for a, b in sym]
    t += [(3, P3[a], P3[b], P3[c]) for a in range(3) for b in range(a, 3) for c in range(b, 3)]
    t += [(0, a, 0, 0) for a in N3]
    assert len(t) == 60
    return t


MONOMIALS = _monomials()


# ---- c. branches and status words ------------------------------------------------------------------------------
N_C, STRIDE_C = 1027, 4        # n = 257: N % stride != 0, two backward blocks


def _healthy(kind, seed, gt=257):
    p, nn, w, _ = make_segment(kind, seed, n=257)
    return (kind, p, nn, w, make_gt(p, gt, seed + 1))


def _bit_identical(A, i, B, j):
    for name in ("dist", "params", "status", "cone_direct", "partial", "jac"):
        assert np.array_equal(getattr(A, name)[i], getattr(B, name)[j]), name
    assert np.array_equal(A.seg_grad(i), B.seg_grad(j))


def test_ridge_flag_per_kind(gpu):
    """params[:, 15] reports the ridge parameter: in use for the cylinder (its circle fit is rank deficient along
    the axis), 0 for plane, sphere and cone.  With 80 % of the memberships at eps as well."""
    for sparse in (False, True):
        segments = []
        for k, kind in enumerate(KIND_NAMES):
            _, p, nn, w, gt = _healthy(kind, 40 + k)
            segments.append((kind, p, nn, sparse_weights(w) if sparse else w, gt))
        clouds, segs = _one_per_shape(segments)
        L = Launch(gpu, clouds, segs, N_C, STRIDE_C, 2)
        for i in range(4):
            check_segment(L, i, clouds, label="sparse" if sparse else "dense")
        assert L.params[2, 15] > 0 and not L.params[[0, 1, 3], 15].any()
        assert not L.cone_direct[:3].any() and L.cone_direct[3] > 0


def test_null_cone(gpu):
    p, nn, w, _ = null_cone_segment(3, 257)
    null = ("cone", p, nn, w, make_gt(p, 63, 7))
    healthy = _healthy("cone", 61)
    clouds, segs = _one_per_shape([null, healthy])
    L = Launch(gpu, clouds, segs, N_C, STRIDE_C, 2, coeffs=[2.0, 3.0])
    assert L.status.tolist() == [2, 0] and L.fit_status.tolist() == [2, 0]
    assert L.params[0, :7].tolist() == [0, 0, 0, 1, 0, 0, 0]
    assert L.cone_direct[0] == 0 and not L.jac[0].any()
    assert not L.seg_grad(0).any()
    ref_p, ref_d, ref_g = oracle("cone", p, nn, segs[0]["w"], null[4], torch.float64)     # the same branch
    assert ref_p.tolist() == [0, 0, 0, 1, 0, 0, 0] and not ref_g.any()
    print("null cone: dist %.4e rel err %.1e" % (ref_d, abs(float(L.dist[0]) - ref_d) / ref_d))
    assert abs(float(L.dist[0]) - ref_d) < 5e-6 * ref_d
    check_segment(L, 1, clouds, label="beside the null cone")
    L.check_untouched_gradient()
    c1, s1 = _one_per_shape([healthy])
    alone = Launch(gpu, c1, s1, N_C, STRIDE_C, 2, coeffs=[3.0])
    _bit_identical(L, 1, alone, 0)


@pytest.mark.parametrize("noise", [0.0, 1e-5])
def test_cone_angle_on_its_clamp(gpu, noise):
    p, nn, w, gt = clamped_cone_segment(1, noise=noise)
    clouds, segs = _one_per_shape([("cone", p, nn, w, gt), _healthy("cone", 62)])
    L = Launch(gpu, clouds, segs, N_C, STRIDE_C, 2)
    assert L.status.tolist() == [0, 0]
    assert L.params[0, 6] == CONE_THETA_MAX
    assert L.cone_direct[0] == 0 and not L.jac[0, 6].any()          # a clamped angle passes no gradient
    assert L.cone_direct[1] > 0 and L.jac[1, 6].any()
    check_segment(L, 0, clouds, dist_tol=CLAMPED_CONE_BARS[noise]["dist"], grad_tol=CLAMPED_CONE_BARS[noise]["grad"],
                  label="clamped")
    check_segment(L, 1, clouds, label="beside the clamped cone")


def test_cone_axis_orientation(gpu):
    """The same cone with all normals negated: the oracle flips the axis, both runs match it.  Exactly one of the
    two takes the `dotn > 0` branch of fit_segment (shown on the CPU by
    tests/test_fit_math_host.py::test_cone_axis_orientation: the Gram matrix of the normals, hence the unoriented
    axis, is the same in both runs, and sum n . a changes sign)."""
    kind, p, nn, w, gt = _healthy("cone", 50)
    clouds, segs = _one_per_shape([(kind, p, nn, w, gt), (kind, p, -nn, w, gt)])
    L = Launch(gpu, clouds, segs, N_C, STRIDE_C, 2)
    for i in range(2):
        check_segment(L, i, clouds, label="normals %+d" % (1 - 2 * i))
    assert np.array_equal(L.params[0, 3:6], -L.params[1, 3:6])
    flipped = [a[np.abs(a).argmax()] < 0 for a in (L.params[0, 3:6], L.params[1, 3:6])]
    assert sorted(flipped) == [False, True]


def test_evaluation_mode_residual(gpu):
    """sqrt_flag: guard_sqrt of every point's squared residual before the mean."""
    segments = [_healthy(kind, 30 + k) for k, kind in enumerate(KIND_NAMES)]
    clouds, segs = _one_per_shape(segments)
    L = Launch(gpu, clouds, segs, N_C, STRIDE_C, 2, sqrt_flag=True, coeffs=[1.0, 2.0, 3.0, 4.0])
    for i in range(4):
        check_segment(L, i, clouds, sqrt=True, label="sqrt")
    plain = Launch(gpu, clouds, segs, N_C, STRIDE_C, 2)
    assert (L.dist > 5 * plain.dist).all()          # root of ~4e-4 against ~4e-4: the flag reached the kernel


def test_sphere_radius_under_its_clamp(gpu):
    kind, p, nn, w, _ = _healthy("sphere", 7)
    tiny = (p * 0.05).astype(np.float32)            # radius^2 ~ 2e-4 < 1e-3
    clouds, segs = _one_per_shape([("sphere", tiny, nn, w, tiny[::2].copy())])
    L = Launch(gpu, clouds, segs, N_C, STRIDE_C, 2)
    assert abs(L.params[0, 3] - np.sqrt(1e-3)) < 1e-12
    check_segment(L, 0, clouds, label="tiny sphere")


def test_non_finite_segment_keeps_to_itself(gpu):
    """A point with an infinite coordinate is bad data, not a fault: the Jacobi sweeps are bounded, the segment
    reports status bit 0 or 2, and the other segments of the launch do not notice."""
    segments = [_healthy("plane", 70), _healthy("sphere", 71), _healthy("cone", 72), _healthy("cylinder", 73),
                _healthy("plane", 74)]
    bad = [list(s) for s in segments]
    for i in (1, 4):                                 # a sphere (lstsq3: bit 0) and a plane (NaN distance: bit 2)
        bad[i][1] = bad[i][1].copy()
        bad[i][1][0, 1] = np.inf
    clouds, segs = _one_per_shape(segments)
    good = Launch(gpu, clouds, segs, N_C, STRIDE_C, 2)
    cb, sb = _one_per_shape([tuple(s) for s in bad])
    L = Launch(gpu, cb, sb, N_C, STRIDE_C, 2)
    assert good.status.tolist() == [0] * 5
    assert L.status[1] & 5 and L.status[4] & 5, L.status
    assert L.status[1] & 1
    for i in (0, 2, 3):
        _bit_identical(L, i, good, i)
        check_segment(L, i, cb, label="beside a non-finite segment")
    L.check_untouched_gradient()          # the bad segments' own entries may hold anything, nothing else is touched


def test_empty_ground_truth(gpu):
    segments = [_healthy("cone", 80), _healthy("cone", 81, gt=0), _healthy("sphere", 82, gt=0),
                _healthy("cylinder", 83)]
    clouds, segs = _one_per_shape(segments)
    L = Launch(gpu, clouds, segs, N_C, STRIDE_C, 2, coeffs=[1.0, 5.0, 7.0, 2.0])
    off = L.tab["gt_off"].cpu().tolist()
    assert off[1] == off[2] == off[3]
    assert L.status.tolist() == [0, 0, 0, 0] and L.fit_status.tolist() == [0, 0, 0, 0]      # unchanged
    for i in (1, 2):
        assert L.dist[i] == 0
        g = L.seg_grad(i)
        assert np.isfinite(g).all() and not g.any()
    assert np.isfinite(L.params).all()
    for i in (0, 3):
        check_segment(L, i, clouds, label="beside empty ground truth")
    L.check_untouched_gradient()


# ---- d. B-spline evaluation off the square grid ---------------------------------------------------------------
def _bspline_case(cu, cv, gu, gv, S, seed):
    g = torch.Generator().manual_seed(seed)
    nu, nv = torch.randn(gu, cu, generator=g), torch.randn(gv, cv, generator=g)
    ctrl = torch.randn(S, cu, cv, 3, generator=g)
    affine = torch.randn(S, 3, 4, generator=g)
    return nu, nv, ctrl, affine


def _bspline_fwd_ref(nu, nv, ctrl, affine, wrap):
    """fp64 value and the same expression on absolute values (the running-error majorant)."""
    nu, nv, ctrl = nu.double(), nv.double(), ctrl.double()
    X = torch.einsum("ui,vj,sijc->suvc", nu, nv, ctrl)
    Xa = torch.einsum("ui,vj,sijc->suvc", nu.abs(), nv.abs(), ctrl.abs())
    if affine is not None:
        A = affine.double()
        X = torch.einsum("scd,suvd->suvc", A[:, :, :3], X) + A[:, None, None, :, 3]
        Xa = torch.einsum("scd,suvd->suvc", A[:, :, :3].abs(), Xa) + A[:, None, None, :, 3].abs()
    if wrap:
        X, Xa = torch.cat([X, X[:, :1]], 1), torch.cat([Xa, Xa[:, :1]], 1)
    S = X.shape[0]
    return X.reshape(S, -1, 3), Xa.reshape(S, -1, 3)


def _bspline_bwd_ref(nu, nv, gout, affine, wrap):
    nu, nv = nu.double(), nv.double()
    S, gu, gv = gout.shape[0], nu.shape[0], nv.shape[0]
    G = gout.double().reshape(S, gu + int(wrap), gv, 3)
    Ga = G.abs()
    if wrap:                                       # the appended row is row 0 again
        G = torch.cat([G[:, :1] + G[:, gu:], G[:, 1:gu]], 1)
        Ga = torch.cat([Ga[:, :1] + Ga[:, gu:], Ga[:, 1:gu]], 1)
    if affine is not None:
        A = affine.double()[:, :, :3]
        G = torch.einsum("scd,suvc->suvd", A, G)
        Ga = torch.einsum("scd,suvc->suvd", A.abs(), Ga)
    return (torch.einsum("ui,vj,suvc->sijc", nu, nv, G),
            torch.einsum("ui,vj,suvc->sijc", nu.abs(), nv.abs(), Ga))


@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("cu,cv,gu,gv", [(10, 12, 40, 17), (4, 7, 5, 9), (20, 20, 30, 30)])
def test_bspline_eval_off_the_square_grid(gpu, cu, cv, gu, gv, S):
    """Dense random nu (gu,cu) and nv (gv,cv) with all four sizes different: a u index taken for a v index shows.
    Bar per element: (cu + cv + 8) eps32 times the expression on absolute values, the bound of two chained fp32
    dot products and the 3x4 map."""
    from parsenet_codebase_amd import kernels as K
    from parsenet_codebase_amd.fitting_batch import _BSplineEval
    torch.cuda.set_device(gpu)
    nu, nv, ctrl, affine = _bspline_case(cu, cv, gu, gv, S, 1000 * cu + S)
    bar = (cu + cv + 8) * EPS32
    d = lambda t: None if t is None else t.to(gpu)      # noqa: E731
    for aff in (affine, None):
        for wrap in (False, True):
            ref, mag = _bspline_fwd_ref(nu, nv, ctrl, aff, wrap)
            out = K.bspline_eval(d(nu), d(nv), d(ctrl), d(aff), wrap)
            assert out.shape == (S, (gu + int(wrap)) * gv, 3)
            ratio = float(((out.cpu().double() - ref).abs() / mag).max())
            gout = torch.randn(ref.shape, generator=torch.Generator().manual_seed(5))
            gref, gmag = _bspline_bwd_ref(nu, nv, gout, aff, wrap)
            gctrl = K.bspline_eval_bwd(d(nu), d(nv), d(gout), d(aff), cu, cv, wrap)
            assert gctrl.shape == (S, cu, cv, 3)
            gratio = float(((gctrl.cpu().double() - gref).abs() / gmag).max())
            print("bspline %s affine=%s wrap=%d: fwd %.2f eps, bwd %.2f eps (bar %d eps)" % (
                (cu, cv, gu, gv, S), aff is not None, wrap, ratio / EPS32, gratio / EPS32, cu + cv + 8))
            assert ratio <= bar and gratio <= bar
            # the same through autograd
            c = d(ctrl).requires_grad_(True)
            o = _BSplineEval.apply(c, d(nu), d(nv), d(aff), wrap)
            assert torch.equal(o, out)
            (o * d(gout)).sum().backward()
            assert torch.equal(c.grad, gctrl)


def test_bspline_lds_guard_refuses_before_launching(gpu):
    from parsenet_codebase_amd import _lib, kernels as K
    torch.cuda.set_device(gpu)
    g = torch.Generator().manual_seed(0)
    # backward: (74*74*3 + 74*2*3) * 4 = 67 488 bytes > 64 KiB
    gu = gv = 74
    cu = cv = 2
    nu, nv = torch.randn(gu, cu, generator=g).to(gpu), torch.randn(gv, cv, generator=g).to(gpu)
    gout = torch.randn(1, gu * gv, 3, generator=g).to(gpu)
    with pytest.raises(RuntimeError, match=r"pn_bspline_eval_bwd_f32: grid too large for the LDS tile \(67488 bytes\)"):
        K.bspline_eval_bwd(nu, nv, gout, None, cu, cv)
    sentinel = torch.full((1, cu, cv, 3), 7.0, device=gpu)
    with _lib.on_device(gpu):
        rc = _lib.load().pn_bspline_eval_bwd_f32(_lib.ptr(nu), _lib.ptr(nv), _lib.ptr(gout), None, 1, gu, gv, cu, cv,
                                                 0, _lib.ptr(sentinel), _lib.current_stream(gpu))
    torch.cuda.synchronize()
    assert rc != 0 and bool((sentinel == 7.0).all())                   # nothing was launched
    # forward: (60*60*3 + 32*60*3) * 4 = 66 240 bytes
    nu, nv = torch.randn(32, 60, generator=g).to(gpu), torch.randn(3, 60, generator=g).to(gpu)
    ctrl = torch.randn(1, 60, 60, 3, generator=g).to(gpu)
    with pytest.raises(RuntimeError, match=r"pn_bspline_eval_f32: grid too large for the LDS tile \(66240 bytes\)"):
        K.bspline_eval(nu, nv, ctrl)
    # just under the limit still runs: (73*73*3 + 73*2*3) * 4 = 65 700 > 64 KiB too; 72: 63 936 bytes
    gu = gv = 72
    nu, nv = torch.randn(gu, cu, generator=g), torch.randn(gv, cv, generator=g)
    gout = torch.randn(1, gu * gv, 3, generator=g)
    gref, gmag = _bspline_bwd_ref(nu, nv, gout, None, False)
    gctrl = K.bspline_eval_bwd(nu.to(gpu), nv.to(gpu), gout.to(gpu), None, cu, cv)
    # (here the dot products run over the grid, 72 + 72 terms, not over 2 + 2 control points)
    assert float(((gctrl.cpu().double() - gref).abs() / gmag).max()) <= (gu + gv + 8) * EPS32


# ---- e. sym3_eig -----------------------------------------------------------------------------------------------
EIG_BAR = 64 * 2.0 ** -53
EIG_FAMILIES = ["spd", "diagonal", "two_equal", "identity", "rank_one", "non_symmetric", "zero"]


def sym3_inputs(family, M, seed):
    rng = np.random.RandomState(seed)
    Q = np.linalg.qr(rng.randn(M, 3, 3))[0]
    if family == "spd":
        A = rng.randn(M, 3, 3)
        return A @ A.transpose(0, 2, 1) + 0.1 * np.eye(3)
    if family == "diagonal":
        return np.einsum("mi,ij->mij", rng.rand(M, 3) + 0.1, np.eye(3))
    if family == "two_equal":
        lam = rng.rand(M, 2) + 0.1
        D = np.einsum("mi,ij->mij", np.stack([lam[:, 0], lam[:, 0], lam[:, 1]], 1), np.eye(3))
        return Q @ D @ Q.transpose(0, 2, 1)
    if family == "identity":
        return (rng.rand(M, 1, 1) + 0.1) * np.eye(3)
    if family == "rank_one":
        v = rng.randn(M, 3)
        return np.einsum("mi,mj->mij", v, v)
    if family == "non_symmetric":
        A = rng.randn(M, 3, 3)
        return A @ A.transpose(0, 2, 1) + 0.1 * np.eye(3) + 0.3 * (A - A.transpose(0, 2, 1))
    return np.zeros((M, 3, 3))


def check_sym3(G, w, V, label=""):
    """Descending order, orthonormality, residual and eigenvalue error relative to |G|_F within 64 * 2^-53, the
    sign convention (largest component of every eigenvector positive) wherever that component is unique."""
    Gs = 0.5 * (G + G.transpose(0, 2, 1))
    F = np.sqrt((Gs ** 2).sum((1, 2)))
    zero = F == 0
    assert (w[:, 0] >= w[:, 1]).all() and (w[:, 1] >= w[:, 2]).all(), label
    orth = np.abs(V.transpose(0, 2, 1) @ V - np.eye(3)).max()
    assert orth <= EIG_BAR, (label, orth)
    if zero.any():
        assert not w[zero].any() and np.array_equal(V[zero], np.broadcast_to(np.eye(3), V[zero].shape))
    nz = ~zero
    if not nz.any():
        return
    ref = torch.linalg.eigvalsh(torch.from_numpy(Gs[nz])).numpy()[:, ::-1]
    res = (np.abs(Gs[nz] @ V[nz] - V[nz] * w[nz][:, None, :]).max((1, 2)) / F[nz]).max()
    err = (np.abs(w[nz] - ref).max(1) / F[nz]).max()
    print("sym3 %s: orth %.1f res %.1f eval %.1f (units of 2^-53, bar 64)" % (
        label, orth * 2.0 ** 53, res * 2.0 ** 53, err * 2.0 ** 53))
    assert res <= EIG_BAR, (label, res)
    assert err <= EIG_BAR, (label, err)
    a = np.sort(np.abs(V), 1)                                  # per column: magnitudes ascending
    unique = (a[:, 2] - a[:, 1]) > EIG_BAR
    big = np.take_along_axis(V, np.abs(V).argmax(1)[:, None, :], 1)[:, 0]
    assert (big[unique] > 0).all(), label


@pytest.mark.parametrize("M", [1, 64, 65, 130])
def test_sym3_eig(gpu, M):
    from parsenet_codebase_amd import kernels as K
    torch.cuda.set_device(gpu)
    for f, family in enumerate(EIG_FAMILIES):
        for scale in ((1.0,) if family == "zero" else (1.0, 1e-12, 1e12)):
            G = sym3_inputs(family, M, 10 * M + f) * scale
            w, V = K.sym3_eig(torch.from_numpy(G).to(gpu))
            assert w.shape == (M, 3) and V.shape == (M, 3, 3)
            check_sym3(G, w.cpu().numpy(), V.cpu().numpy(), "%s x %g M=%d" % (family, scale, M))
    # a mixed batch: every thread of a block on another family
    G = np.concatenate([sym3_inputs(fam, 1, 7 * M + t) for t, fam in
                        zip(range(M), EIG_FAMILIES * (M // len(EIG_FAMILIES) + 1))])
    w, V = K.sym3_eig(torch.from_numpy(G).to(gpu))
    check_sym3(G, w.cpu().numpy(), V.cpu().numpy(), "mixed M=%d" % M)
