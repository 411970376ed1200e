"""The ragged batch of the raw-cloud kernels as a value.

A caller hands over one cloud (N,3), a batch (B,N,3) or a list of (N_b,3) tensors; the kernels of ``kernels.py`` want a
flat (total,3) array and the offsets of its segments, and the caller wants the results back the way the clouds came.
``Clouds`` is built once per public call and is the one place where the clouds are flattened, where the offsets are
formed and uploaded (once: every kernel of the call reads the same device tensor), where an array that runs beside the
points is held to their layout, and where results find their way back."""
import numpy as np
import torch

from . import _lib


class Clouds:
    """layout   "single", "list", or the shape (B, N) of a batch
    sizes    points per cloud, a list of S integers (a batch: N, B times)
    flat     (total,3) fp32, the clouds one after another (a view where the input allows it)
    off      the host offsets, (S+1) int64: off[s] .. off[s+1] - 1 are the rows of cloud s
    S, total, max_n   the number of clouds, of points, and of points in the largest cloud"""

    def __init__(self, points, who, bad_dtype=ValueError, on_gpu=True):
        """points: (N,3), (B,N,3) or a list of (N_b,3) fp32 tensors on the GPU.  ``who`` names the caller in the
        errors; a dtype other than fp32 raises ``bad_dtype``; ``on_gpu=False`` skips the device check (the shape logic
        runs on any tensor: tests/test_ragged_host.py)."""
        if isinstance(points, (list, tuple)):
            clouds = list(points)
            if not clouds:
                raise ValueError("%s: an empty list of clouds" % who)
            if not all(torch.is_tensor(c) for c in clouds):
                raise TypeError("%s: a list of clouds holds tensors" % who)
            self.layout = "list"
        elif torch.is_tensor(points):
            clouds = [points]
            self.layout = "single" if points.dim() == 2 else "batch"
        else:
            raise TypeError("%s: points must be a tensor or a list of tensors" % who)
        self._on_gpu = on_gpu
        if on_gpu:
            _lib.require_cuda(*clouds)
        for c in clouds:
            if c.dtype != torch.float32:
                raise bad_dtype("%s: points must be float32, got %s" % (who, c.dtype))
            if c.dim() != (3 if self.layout == "batch" else 2) or c.shape[-1] != 3:
                raise ValueError("%s: points must be (N,3), (B,N,3) or a list of (N,3), got %s"
                                 % (who, tuple(c.shape)))
        if self.layout == "batch":
            B, N = points.shape[:2]
            self.layout, self.sizes, self.flat = (B, N), [N] * B, points.reshape(B * N, 3)
        else:
            self.sizes = [c.shape[0] for c in clouds]
            self.flat = clouds[0] if len(clouds) == 1 else torch.cat(clouds)
        self.off = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        self.S, self.total, self.max_n = len(self.sizes), int(self.off[-1]), max(self.sizes, default=0)
        self._device_off = None

    def device_offsets(self):
        """The offsets on the device of the points, (S+1) int32: uploaded at the first call (one stream-ordered copy),
        the same tensor from then on."""
        if self._device_off is None:
            self._device_off = _lib.h2d(self.off.astype(np.int32), self.flat.device)
        return self._device_off

    def beside(self, array, who, what):
        """An array with one row per point — normals, colours, labels; (N,...), (B,N,...) or a list of (N_b,...) — as
        (total,...) in the order of ``flat``.  It must come in the layout and the sizes of the points (ValueError);
        ``who`` and ``what`` name the caller and the array in the errors."""
        parts = list(array) if isinstance(array, (list, tuple)) else [array]
        if not all(torch.is_tensor(a) for a in parts):
            raise TypeError("%s: %s must be a tensor or a list of tensors" % (who, what))
        if self._on_gpu:
            _lib.require_cuda(*parts)
        if isinstance(array, (list, tuple)):
            same = self.layout == "list" and [int(a.shape[0]) if a.dim() else -1 for a in parts] == self.sizes
        elif isinstance(self.layout, tuple):
            same = tuple(array.shape[:2]) == self.layout
        else:
            same = self.layout == "single" and array.dim() >= 1 and array.shape[0] == self.sizes[0]
        if not same:
            raise ValueError("%s: %s must have the same layout and sizes as the points" % (who, what))
        if isinstance(self.layout, tuple):
            return array.reshape((-1,) + tuple(array.shape[2:]))
        return array if self.layout == "single" else parts[0] if len(parts) == 1 else torch.cat(parts)

    def per_point(self, flat):
        """A (total,...) result in the layout of the points: (N,...), (B,N,...) or a list of (N_b,...)."""
        if isinstance(self.layout, tuple):
            return flat.reshape(self.layout + tuple(flat.shape[1:]))
        return list(torch.split(flat, self.sizes)) if self.layout == "list" else flat

    def per_cloud(self, rows):
        """(S,m,...) rows, m per cloud, in the layout of the points: (m,...), (B,m,...) or a list of (m,...)."""
        if isinstance(self.layout, tuple):
            return rows
        return list(rows.unbind(0)) if self.layout == "list" else rows[0]
