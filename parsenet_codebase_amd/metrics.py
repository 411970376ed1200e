"""Evaluation metrics of the reference's test.py:39-47, 157-185 on the HIP Chamfer kernel:
surface coverage (s-k), point coverage (p-k), their thresholds at 1 % and 2 % of the unit box,
and the symmetric Chamfer figure the paper reports; plus segment / primitive-type IoU
(``SIOU_matched_segments``) and the per-point primitive mIoU (``evaluate_miou``) re-exported; and the point coverage of the fitted
primitives of src/eval_utils.py:103-127 (``p_coverage``)."""
import os

import numpy as np
import torch

from . import kernels as K
from ._lib import h2d
from .chamfer import chamfer_distance_single_shape
from .fitting import SIOU_matched_segments  # noqa: F401
from .losses import evaluate_miou  # noqa: F401


def continuous_labels(labels_):
    """test.py:39-47: relabel to 0..K-1 in order of np.unique."""
    labels_ = np.asarray(labels_)
    return np.unique(labels_, return_inverse=True)[1].reshape(labels_.shape).astype(labels_.dtype)


def coverage_metrics(pred_points, points):
    """pred_points (M,3): samples of the reconstructed surfaces; points (N,3): the input cloud.
    cd1[i] = distance of input point i to the nearest sample (how well the surfaces cover the
    shape, "s"), cd2[j] = distance of sample j to the nearest input point ("p"); both with
    guard_sqrt, like test.py:157-160.  Returns the dict test.py:172-180 builds (without the IoUs)."""
    pred_points = torch.as_tensor(pred_points)
    points = torch.as_tensor(points)
    cd1 = chamfer_distance_single_shape(pred_points, points, sqrt=True, one_side=True, reduce=False)
    cd2 = chamfer_distance_single_shape(points, pred_points, sqrt=True, one_side=True, reduce=False)
    sk, pk = torch.mean(cd1).item(), torch.mean(cd2).item()
    return {"sk_1": torch.mean((cd1 < 0.01).float()).item(), "sk_2": torch.mean((cd1 < 0.02).float()).item(),
            "sk": sk, "pk_1": torch.mean((cd2 < 0.01).float()).item(),
            "pk_2": torch.mean((cd2 < 0.02).float()).item(), "pk": pk, "cd": (sk + pk) / 2.0}


def coverage_rows(pred, pts):
    """pred[b] (M_b,3), pts[b] (N_b,3): fp32 tensors on the GPU -> one dict per shape (the keys of
    ``coverage_metrics``).  ONE ragged nearest-neighbour call for both sides of all shapes, ONE reduction
    (csrc/chamfer.hip, pn_coverage_reduce_f32: fp32 roots and comparisons, fp64 sums in a fixed order), ONE download
    of the (S,6) table; means and cd are formed here in float64."""
    dev = pts[0].device
    na = np.asarray([p.shape[0] for p in pts], np.int64)
    nb = np.asarray([p.shape[0] for p in pred], np.int64)
    if na.sum() >= 2 ** 31 or nb.sum() >= 2 ** 31:
        raise ValueError("coverage_metrics_batch: int32 offsets")
    S = na.shape[0]
    table = h2d(np.concatenate([[0], np.cumsum(na), [0], np.cumsum(nb)]).astype(np.int32), dev)
    off_a, off_b = table[:S + 1], table[S + 1:]
    a = pts[0] if S == 1 else torch.cat(pts)
    b = pred[0] if S == 1 else torch.cat(pred)
    minA, _, minB, _ = K.chamfer_nn_ragged(a, off_a, int(na.max()), b, off_b, int(nb.max()))
    t = K.coverage_reduce(minA, off_a, minB, off_b).cpu().numpy()
    out = []
    for s in range(S):
        n, m = float(na[s]), float(nb[s])
        sk, pk = t[s, 0] / n, t[s, 3] / m
        out.append({"sk_1": t[s, 1] / n, "sk_2": t[s, 2] / n, "sk": sk, "pk_1": t[s, 4] / m, "pk_2": t[s, 5] / m,
                    "pk": pk, "cd": (sk + pk) / 2.0})
    return out


def coverage_metrics_batch(pred_points_list, points_list):
    """``coverage_metrics`` of S shapes — pred_points_list[s] (M_s,3) samples of the reconstructed surfaces,
    points_list[s] (N_s,3) the input cloud, arrays or tensors — in three launches and one download (coverage_rows).
    A shape's figures do not depend on the batch it is evaluated in.  Python floats formed in float64: the shares are
    count / size, the means within the fp32 rounding of torch.mean of ``coverage_metrics``."""
    if len(pred_points_list) != len(points_list) or len(points_list) < 1:
        raise ValueError("coverage_metrics_batch: %d sample sets for %d clouds" % (len(pred_points_list),
                                                                                  len(points_list)))
    dev = torch.device("cuda", torch.cuda.current_device())
    both = []
    for name, lst in (("pred_points", pred_points_list), ("points", points_list)):
        row = []
        for s, p in enumerate(lst):
            p = _dev32(p, dev).contiguous()
            if p.dim() != 2 or p.shape[1] != 3 or p.shape[0] < 1:
                raise ValueError("coverage_metrics_batch: shape %d: %s must be (N,3) with N >= 1, got %s"
                                 % (s, name, tuple(p.shape)))
            row.append(p)
        both.append(row)
    return [{k: float(v) for k, v in r.items()} for r in coverage_rows(both[0], both[1])]


def surface_coverage_batch(points_list, surfaces_list):
    """The deterministic limit of the s-coverage figures ``coverage_metrics`` forms from the nearest SAMPLE of the
    reconstruction (sk_1: the share of input points within 0.01 of it, sk: their mean distance): the same figures
    from the distance to the nearest TRIANGLE of the trimmed surfaces (surface.point_surface_distance, one record
    and one distance launch for the batch).  Per shape {"p_cover_surface", "p_dist_surface"}: guard_sqrt of the
    squared distance, the share of roots < 0.01 and the mean root, both formed in float64.  One download."""
    from . import surface
    from .fitting import guard_sqrt
    rows = []
    for d2 in surface.point_surface_distance(points_list, surfaces_list):
        root = guard_sqrt(d2)
        rows.append(torch.stack([(root < 0.01).double().mean(), root.double().mean()]))
    table = torch.stack(rows).cpu().numpy()
    return [{"p_cover_surface": float(r[0]), "p_dist_surface": float(r[1])} for r in table]


def surface_coverage(points, surfaces):
    """``surface_coverage_batch`` of one shape."""
    return surface_coverage_batch([points], [surfaces])[0]


# ---------------------------------------------------------------------------------------
# src/segment_utils.py: the remaining segmentation metrics and membership helpers
# ---------------------------------------------------------------------------------------
def mean_IOU_one_sample(pred, gt, C):
    """segment_utils.py:126-136: mean IoU of the label sets 0..C-1 (empty classes count as 1)."""
    pred, gt = np.asarray(pred), np.asarray(gt)
    eps = np.finfo(np.float32).eps
    total = 0.0
    for c in range(C):
        a, b = gt == c, pred == c
        total += (np.sum(a & b) + eps) / (np.sum(a | b) + eps)
    return total / C


def iou_segmentation(pred, gt):
    """segment_utils.py:267-280: primitive-type IoU after merging 0/6/7 -> 9 and 8 -> 2 (on copies;
    the reference rewrites its arguments in place)."""
    from .fitting import _merge_types
    return mean_IOU_one_sample(_merge_types(pred), _merge_types(gt), 6)


def matching_iou(matching, predicted_labels, labels):
    """segment_utils.py:295-324: mean IoU over the matched (predicted, ground-truth) label pairs."""
    per_shape = []
    for b in range(labels.shape[0]):
        rows, cols = matching[b]
        vals = []
        for r, c in zip(rows, cols):
            p, g = predicted_labels[b] == r, labels[b] == c
            if np.sum(g) == 0 and np.sum(p) == 0:
                continue
            vals.append(np.sum(p & g) / (np.sum(p | g) + 1e-8))
        per_shape.append(np.mean(vals))
    return np.mean(per_shape)


def SIOU(target, pred_labels):
    """fitting_utils.py:336-359: Hungarian matching on the relaxed IoU, then matching_iou."""
    from .fitting import _relaxed_iou_of_labels, solve_dense
    rids, cids = solve_dense(1.0 - _relaxed_iou_of_labels(pred_labels, target).astype(np.float64))
    return matching_iou([[rids, cids]], np.expand_dims(pred_labels, 0), np.expand_dims(target, 0))


def relaxed_iou(pred, gt, max_clusters=50):
    """segment_utils.py:327-353 (the loop form; same values as relaxed_iou_fast)."""
    from .fitting import relaxed_iou_fast
    return relaxed_iou_fast(pred, gt, max_clusters)


def primitive_type_segment(pred, weights):
    """segment_utils.py:245-253: arg-max over types of sum_n pred[n,l] * weights[n,k] (numpy)."""
    return np.argmax(np.asarray(pred).T @ np.asarray(weights), 0)


def primitive_type_segment_torch(pred, weights):
    """segment_utils.py:256-264."""
    return torch.max(pred.transpose(0, 1) @ weights, 0)[1]


def dot_product_from_cluster_centers(embedding, centers):
    return centers @ embedding.T


def cluster_prob(embedding, centers, band_width):
    """segment_utils.py:52-60 (the second, effective definition): Gaussian membership, numpy."""
    dist = 2 - 2 * centers @ embedding.T
    return np.exp(-dist / 2 / band_width) / np.sqrt(2 * np.pi * band_width)


def cluster_prob_mutual(embedding, centers, bandwidth, if_normalize=False):
    """segment_utils.py:63-76."""
    dist = np.exp(centers @ embedding.T / bandwidth)
    prob = dist / np.sum(dist, 0, keepdims=True)
    if if_normalize:
        prob = prob - np.min(prob, 1, keepdims=True)
        prob = prob / np.max(prob, 1, keepdims=True)
    return prob


# ---------------------------------------------------------------------------------------
# src/eval_utils.py: point coverage of the fitted primitives, and its separate_losses
# ---------------------------------------------------------------------------------------
# PARSENET_PCOVER: "fused" = all primitives of all shapes in one launch (csrc/cover.hip); "tensor" = the reference's
# form, one ResidualLoss(one_side=True, reduce=False) call per primitive, stack, min.  fused is opt-in until
# tools/pcover_ab.py has been run on an MI355X and shows it faster at every size (profiles/pcover_ab.txt).
DEFAULT_PCOVER = "tensor"
CALLS_PCOVER = {"fused": 0, "tensor": 0}      # shapes served, by path
_PCOVER_TYPES = {"plane": (0, 4), "sphere": (1, 4), "cylinder": (2, 7), "cone": (3, 7),
                 "open-spline": (K.COVER_SAMPLED, 0), "closed-spline": (K.COVER_SAMPLED, 0)}


def pcover_path():
    name = os.environ.get("PARSENET_PCOVER", DEFAULT_PCOVER)
    if name not in CALLS_PCOVER:
        raise ValueError("PARSENET_PCOVER must be one of %s, got %r" % (sorted(CALLS_PCOVER), name))
    return name


def _dev32(x, dev):
    if torch.is_tensor(x):
        return x.detach().to(device=dev, dtype=torch.float32)
    return h2d(np.asarray(x, np.float32), dev)


def _pcover_tensor(pts, live, residual_cls):
    """The per-primitive path: (dmin (N,), position of the nearest primitive in ``live``)."""
    prm = dict(live)
    dist = residual_cls(one_side=True, reduce=False).residual_loss({k: pts for k in prm}, prm, sqrt=True)
    dmin, arg = torch.min(torch.stack([v[1] for v in dist.values()], 0), 0)
    return dmin, arg


def _pcover_fused(pts, lives):
    """pts: list of (N_b,3) fp32 device tensors; lives: per shape the (key, entry) pairs that are not None.
    ONE launch for every non-torus primitive of every shape; -> per shape (dmin, position in ``live``)."""
    from .fitting import ComputePrimitiveDistance
    dev = pts[0].device
    # The parameter table is packed on the host and uploaded once.  Values that already live on a device are not
    # downloaded (a synchronisation each): they are concatenated once and put into the table by one indexed
    # assignment whose positions come from the host.
    samp, types, nsamp, nprim, slots, torus = [], [], [], [], [], []
    host_val, host_pos, dev_val, dev_pos = [], [], [], []
    for b, live in enumerate(lives):
        pos = []
        for i, (_, v) in enumerate(live):
            if v[0] == "torus":                     # no fit and no slot in the kernel: merged after the launch
                torus.append((b, i, v))
                continue
            t, width = _PCOVER_TYPES[v[0]]
            pos.append(i)
            at = len(types) * K.FIT_NPAR
            types.append(t)
            if t == K.COVER_SAMPLED:
                c = _dev32(v[1][0], dev).reshape(-1, 3)  # params[0][0]: the samples distance_from_bspline takes
                samp.append(c)
                nsamp.append(c.shape[0])
                continue
            nsamp.append(0)
            end = at + width
            for x in v[1:]:
                if torch.is_tensor(x) and x.is_cuda:
                    x = x.detach().reshape(-1)
                    n = x.numel()
                    dev_val.append(x.to(device=dev, dtype=torch.float32))
                    dev_pos.append(np.arange(at, at + n))
                else:
                    x = (x.detach().numpy() if torch.is_tensor(x) else np.asarray(x)).astype(np.float32).reshape(-1)
                    n = x.size
                    host_val.append(x)
                    host_pos.append(np.arange(at, at + n))
                at += n
            if at != end:
                raise ValueError("p_coverage: a %s entry with %d parameter values (%d expected)"
                                 % (v[0], at - (end - width), width))
        slots.append(pos)
        nprim.append(len(pos))
    pt_off = np.concatenate([[0], np.cumsum([p.shape[0] for p in pts])])
    if types:
        table = np.zeros(len(types) * K.FIT_NPAR, np.float32)
        if host_val:
            table[np.concatenate(host_pos)] = np.concatenate(host_val)
        table = h2d(table, dev)
        if dev_val:
            table[h2d(np.concatenate(dev_pos).astype(np.int64), dev)] = torch.cat(dev_val)
        dmin, arg = K.point_primitive_min(
            pts[0] if len(pts) == 1 else torch.cat(pts), pt_off, np.concatenate([[0], np.cumsum(nprim)]), types,
            table.reshape(-1, K.FIT_NPAR), torch.cat(samp) if samp else None,
            np.concatenate([[0], np.cumsum(nsamp)]))
    else:
        dmin = torch.full((int(pt_off[-1]),), float("inf"), dtype=torch.float32, device=dev)
        arg = torch.full((int(pt_off[-1]),), -1, dtype=torch.int32, device=dev)
    arg = arg.clamp_min(0)                          # (-1: see below)
    out = []
    for b, live in enumerate(lives):
        d, a = dmin[pt_off[b]:pt_off[b + 1]], arg[pt_off[b]:pt_off[b + 1]].long()
        if len(pts) > 1:
            # own storage: the order in which torch.mean adds depends on the alignment of the slice, and a shape's
            # figures must not depend on the batch it was evaluated in
            d = d.clone()
        # kernel index -> position in live.  The kernel reports -1 where nothing compared smaller than inf: a shape
        # without kernel primitives (torus entries only), or distances that are all inf.  -1 is read as kernel index
        # 0 (torch.min over an all-inf stack also reports its first row), and a shape without kernel primitives
        # starts at its first entry, so the index stays inside ``live`` even when a torus distance is NaN.
        if len(slots[b]) != len(live):
            a = h2d(np.asarray(slots[b] or [0], np.int64), dev)[a]
        out.append([d, a])
    cp = ComputePrimitiveDistance(reduce=False, one_side=True)
    for b, i, v in torus:                           # the lowest position wins on equal values here too
        d, a = out[b]
        dt = cp.distance_from_torus(pts[b], v[1:], sqrt=True).reshape(-1)
        out[b] = [torch.minimum(d, dt), torch.where((dt < d) | ((dt == d) & (i < a)), torch.full_like(a, i), a)]
    return out


def p_coverage_batch(points, parameters_list, return_points=False, ResidualLoss=None):
    """``p_coverage`` of B shapes; with PARSENET_PCOVER=fused ONE launch serves them all.  points: a list of (N_b,3)
    arrays or tensors (the shapes may differ in size) or one (B,N,3); parameters_list: one dict per shape.
    Returns a list of (mean_coverage, cover); with ``return_points`` of (mean_coverage, cover, dmin (N_b,) fp32,
    key (N_b,) int64: the dict key of the nearest primitive, the earliest entry on equal distances)."""
    path = pcover_path()
    lives = []
    for prm in parameters_list:
        live = [(k, v) for k, v in prm.items() if v is not None]
        if not live:
            raise ValueError("p_coverage: no fitted primitive (an empty dict, or None entries only)")
        for _, v in live:
            if v[0] != "torus" and v[0] not in _PCOVER_TYPES:
                raise ValueError("p_coverage: unknown primitive type %r" % (v[0],))
        lives.append(live)
    if not lives or len(points) != len(lives):
        raise ValueError("p_coverage_batch: %d point clouds for %d parameter dicts" % (len(points), len(lives)))
    pts = []
    for p in points:
        p = torch.from_numpy(np.asarray(p, np.float32)).cuda() if not torch.is_tensor(p) else p.detach().float().cuda()
        if p.dim() != 2 or p.shape[1] != 3 or p.shape[0] < 1:
            raise ValueError("p_coverage: points must be (N,3), got %s" % (tuple(p.shape),))
        pts.append(p.contiguous())
    CALLS_PCOVER[path] += len(lives)
    if path == "fused":
        res = _pcover_fused(pts, lives)
    else:
        if ResidualLoss is None:
            from .fitting import ResidualLoss
        res = [_pcover_tensor(p, live, ResidualLoss) for p, live in zip(pts, lives)]
    out = []
    for (dmin, arg), live in zip(res, lives):
        row = (torch.mean(dmin), torch.mean((dmin < 0.01).float()))
        if return_points:
            keys = [k for k, _ in live]
            if not all(isinstance(k, (int, np.integer)) for k in keys):
                raise TypeError("p_coverage_batch(return_points=True) needs integer dict keys")
            row = row + (dmin, h2d(np.asarray(keys, np.int64), dmin.device)[arg])
        out.append(row)
    return out


def p_coverage(points, parameters, ResidualLoss=None):
    """eval_utils.py:103-127: for every input point the distance to the nearest predicted primitive (analytic for
    plane, sphere, cylinder, cone and torus, sample-based for the splines; sqrt=True).  points (N,3) numpy array or
    tensor; parameters: the dict fitter.fitting.parameters / residual_eval_mode returns (None entries are skipped;
    none left raises ValueError where the reference fails in torch.stack).  ``ResidualLoss``: the reference passes
    its class; the per-primitive path (PARSENET_PCOVER=tensor) uses it when given.
    Returns (mean_coverage, cover): the mean distance and the share of points under 0.01, 0-d tensors."""
    return p_coverage_batch([points], [parameters], ResidualLoss=ResidualLoss)[0]


def separate_losses(distance, gt_points, lamb=1.0):
    """eval_utils.py:130-175: Evaluation.separate_losses, which here also skips the segments with fewer than 100
    ground-truth points."""
    from .fitting import Evaluation
    kept = {k: v for k, v in gt_points.items() if v is not None and v.shape[0] >= 100}
    return Evaluation.separate_losses(None, distance, kept, lamb=lamb)
