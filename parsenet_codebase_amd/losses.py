"""Training losses of the segmentation network (src/segment_loss.py)."""
import os
import weakref

import numpy as np
import torch

from . import kernels as K
from ._lib import h2d
import torch.nn.functional as F


# Opt-in: measured on one box (tools/jobs/r6p.sh, two processes each way) the shared node made the cfg5 step SLOWER,
# 177.8 against 180.7 shapes/s, with the same mean-shift launch durations — fewer kernels but a different order of
# the backward nodes around the step's host synchronisation points.  Off by default.
SHARE_NORMALIZE = os.environ.get("PARSENET_SHARE_NORMALIZE", "0") != "0"
_NORMALIZED = []          # at most one entry: weak references to the source's base and to the result, version, view geometry


def normalized_rows(x):
    """torch.nn.functional.normalize(x, p=2, dim=2), evaluated ONCE per tensor when SHARE_NORMALIZE is set.  The embedding loss
    (src/segment_loss.py:45) and the fitting stage (src/residual_utils.py:108) both normalise the network's embedding — the
    same tensor expression on the same view twice a step, forward and backward (~0.08 ms on 4 x 10 000 x 128).  The
    second caller gets the first caller's result (same bits; its gradient reaches the embedding through one
    normalisation node instead of two).  The entry is keyed by the identity of the underlying tensor (a weak
    reference: a freed tensor never matches), its version counter (an in-place write invalidates it), the view's
    geometry and the autograd mode; it holds the result weakly (alive as long as the first user's graph is).
    Both users must take part in the SAME backward pass, as the end-to-end step's single ``loss.backward()`` does: a backward pass in between frees the shared node and the second one raises
    autograd's "backward through the graph a second time" (PARSENET_SHARE_NORMALIZE=1 turns the sharing on)."""
    if not SHARE_NORMALIZE or x.dim() != 3:
        return torch.nn.functional.normalize(x, p=2, dim=2)
    base = x._base if x._base is not None else x
    mode = bool(torch.is_grad_enabled() and x.requires_grad)
    geo = (tuple(x.shape), tuple(x.stride()), x.storage_offset(), x.dtype, mode)
    if _NORMALIZED:
        ref, ver, g, rres = _NORMALIZED[0]
        res = rres()                 # (weak: the entry keeps neither the 20 MB result nor its graph alive)
        if res is not None and ref() is base and ver == base._version and g == geo:
            return res
    res = torch.nn.functional.normalize(x, p=2, dim=2)
    _NORMALIZED[:] = [(weakref.ref(base), base._version, geo, weakref.ref(res))]
    return res


FUSED = True        # False: the tensor-expression form of the same arithmetic (tests compare the two)
TRIPLET_WIDTHS = (32, 64, 128)     # embedding widths csrc/fused.hip's triplet kernels are instantiated for
CALLS_TRIPLET_FUSED = 0            # groups of sampled segment pairs that ran the fused triplet kernels


def triplet_width(D):
    """The width a D-wide embedding runs the fused triplet kernels at (zero-padded up to it), None above 128."""
    for W in TRIPLET_WIDTHS:
        if D <= W:
            return W
    return None


class _TripletItems(torch.autograd.Function):
    """The arithmetic of src/segment_loss.py:97-121 for ALL sampled segment pairs of a batch in one
    launch (csrc/fused.hip): flat (rows,D) unit-row embedding, D = 32, 64 or 128, ia / ib (P,num) row indices of the
    anchor-positive / negative samples, w (P,) = 1 / (pairs of the shape + 1e-8) -> sum over the
    items of w * (sum_ij c_ij - sum_i c_ii) / (#(c > 0) + 1), the count detached like the reference."""

    @staticmethod
    def forward(ctx, flat, ia, ib, w, margin):
        flat = flat.contiguous()
        loss, scale = K.triplet_fwd(flat, ia, ib, w, margin)
        ctx.save_for_backward(flat, ia, ib, scale)
        ctx.margin = margin
        return loss

    @staticmethod
    def backward(ctx, g):
        flat, ia, ib, scale = ctx.saved_tensors
        return K.triplet_bwd(flat, ia, ib, scale, g.contiguous(), ctx.margin), None, None, None, None


class EmbeddingLoss:
    """src/segment_loss.py:20-124.  Same sampling (numpy RNG, same call order, so a seeded run
    draws the same triplets as the reference), but the <= 25 segment pairs of a shape are
    evaluated as one batched tensor expression instead of a Python loop of tiny kernels."""

    def __init__(self, margin=1.0, if_mean_shift=False):
        self.margin = margin
        self.if_mean_shift = if_mean_shift

    def triplet_loss(self, output, labels, iterations=5):
        """output (B,D,N) embedding, labels (B,N) integer array -> loss tensor of shape (1,)."""
        max_segments = 5
        B, _, N = output.shape
        dev = output.device
        labels = np.asarray(labels)
        out = normalized_rows(output.permute(0, 2, 1))          # (shared with the fitting stage of the same step)
        if self.if_mean_shift:
            from .mean_shift import MeanShift
            ms = MeanShift()
            out = torch.stack([ms.mean_shift(out[b], 4000, 0.015, iterations=iterations, nms=False)[0]
                               for b in range(B)], 0)

        # phase 1 (reference :62-76): sample points of every segment of every shape
        samples = []
        for i in range(B):
            p = labels[i]
            uniq = np.unique(p)
            num = min([N // uniq.shape[0] + 1, 30])
            per_label = []
            for l in uniq:
                ids = np.where(p == l)[0]
                per_label.append(np.random.choice(ids, num, replace=True))
            samples.append(np.stack(per_label, 0))            # (S_i, num)

        # phase 2 (reference :85-123): random ordered segment pairs per shape; the RNG draws happen
        # in the reference's order, the arithmetic of ALL pairs of ALL shapes is one batched
        # expression (every shape samples the same number of points per segment when
        # N // S + 1 >= 30, the usual case; otherwise shapes are grouped by sample count)
        only_one = 0
        pair_sets = []          # (shape, pairs (P,2), normalization)
        for i in range(B):
            S = samples[i].shape[0]
            if S == 1:
                only_one += 1
                continue
            num_iterations = min([max_segments * max_segments, S * S])
            pairs = []
            for _ in range(num_iterations):
                k1 = np.random.choice(S, 1)[0]
                k2 = np.random.choice(S, 1)[0]
                if k1 != k2:
                    pairs.append((k1, k2))
            if pairs:
                pair_sets.append((i, np.asarray(pairs), len(pairs)))
        loss_diff = torch.zeros(1, device=dev)
        by_num = {}
        for i, pairs, norm in pair_sets:
            by_num.setdefault(samples[i].shape[1], []).append((i, pairs, norm))
        for num, group in by_num.items():
            ia, ib, wts = [], [], []
            for i, pairs, norm in group:
                ia.append(i * N + samples[i][pairs[:, 0]])           # (P,num) flat point indices
                ib.append(i * N + samples[i][pairs[:, 1]])
                wts.append(np.full(len(pairs), 1.0 / (norm + 1e-8), dtype=np.float32))
            ia = h2d(np.concatenate(ia, 0), dev)
            ib = h2d(np.concatenate(ib, 0), dev)
            wts = h2d(np.concatenate(wts, 0), dev)
            flat = out.reshape(B * N, -1)
            W = triplet_width(flat.shape[1])
            if FUSED and flat.is_cuda and W is not None and num <= 32:
                # widths between the kernels' are zero-padded to the next one: the squared difference of two zero
                # columns is zero, and the pad hands the gradient's first D columns back
                global CALLS_TRIPLET_FUSED
                CALLS_TRIPLET_FUSED += 1
                flat_w = flat if W == flat.shape[1] else F.pad(flat, (0, W - flat.shape[1]))
                loss_diff = loss_diff + _TripletItems.apply(flat_w, ia, ib, wts, float(self.margin))
                continue
            # embeddings wider than 128: the same arithmetic as tensor expressions
            p1, p2 = flat[ia], flat[ib]                              # (P,num,D)
            anchor = p1.unsqueeze(2)
            diff_pos = ((anchor - p1.unsqueeze(1)) ** 2).sum(3)      # (P,num,num)
            diff_neg = ((anchor - p2.unsqueeze(1)) ** 2).sum(3)
            constraint = F.relu(diff_pos - diff_neg + self.margin)
            loss = constraint.sum((1, 2)) - torch.diagonal(constraint, dim1=1, dim2=2).sum(1)
            satisfied = ((constraint > 0).sum((1, 2)) + 1.0).to(loss.dtype)
            loss_diff = loss_diff + ((loss / satisfied.detach()) * wts).sum()
        return loss_diff / (B - only_one + 1e-8)


def evaluate_miou(gt_labels, pred_labels):
    """src/segment_loss.py:127-148 (numpy, metrics only)."""
    N = gt_labels.shape[0]
    C = pred_labels.shape[2]
    pred = np.argmax(pred_labels, 2)
    eps = np.finfo(np.float32).eps
    total = 0.0
    for n in range(N):
        part = 0.0
        for c in range(C):
            g = gt_labels[n] == c
            p = pred[n] == c
            part += (np.sum(g & p) + eps) / (np.sum(g | p) + eps)
        total += part / C
    return total / N


def primitive_loss(pred, gt):
    """src/segment_loss.py:151-152: nn.NLLLoss() (mean) of pred (B,K,N) log-probabilities at gt (B,N).
    Written as gather + mean: torch's nll_loss2d forward accumulates with atomics on the GPU (its
    result is not reproducible run to run); every target selects one entry, so the gather's backward
    has no collisions and the mean is a fixed-order reduction."""
    if pred.dim() == 3 and pred.is_cuda:
        return -torch.gather(pred, 1, gt.long().unsqueeze(1)).mean()
    return F.nll_loss(pred, gt)
