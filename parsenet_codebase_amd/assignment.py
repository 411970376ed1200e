"""Linear sum assignment with the heavy part on the GPU: a batched auction (csrc/lsa.hip) leaves column prices
that are eps-optimal duals, and the host finishes from them EXACTLY.

The evaluation-mode LS refit (src/primitive_forward.py:197-198, 272-273) matches 1 600 surface samples to 1 600 ...
2 100 input points per spline segment with lapsolver.solve_dense; scipy's linear_sum_assignment on the raw matrix
is what the host path (``fitting.solve_dense``) runs.  An auction result is only eps-optimal and the refit is held
to the optimal permutation itself, so the device path uses the auction for what it is good at — prices — and lets
scipy finish on the REDUCED matrix: for any prices p, with u_i = min_j (c_ij + p_j),

    R_ij = c_ij - u_i + p_j  >=  0,

and on a square problem R and c have the same optimal assignments (every assignment's cost moves by the constant
sum p - sum u).  The shortest-augmenting-path solver then works in time that grows with how far p is from optimal
duals instead of O(n^3).  A rectangular problem (n < m) is reduced on the padded square, as the kernel solves it:
the m - n zero-cost rows get R_dj = p_j - min_j p_j.  Reducing the real rows alone is NOT equivalent (a column's
price then shifts the cost of exactly those assignments that use the column).

This module imports numpy and scipy only at the top: ``finish_exact`` runs in the spawned workers of
``fitting_eval.assignment_pool()``, which never touch torch or the GPU.

``PARSENET_REFIT_LSA`` = ``host`` (default: scipy on the raw matrix, the assignment pool) | ``device`` routes the
refit's matchings; ``CALLS_LSA`` counts them."""
import os

import numpy as np
from scipy.optimize import linear_sum_assignment


def _mode_from_env():
    return os.environ.get("PARSENET_REFIT_LSA", "host")


REFIT_LSA = _mode_from_env()
CALLS_LSA = {"device": 0, "host": 0, "capped": 0}        # matchings of the refit by the path that solved them

# The auction's schedule (fractions of the cost range) and its round cap.  They are to be chosen from the record of
# tools/lsa_device_ab.py (profiles/lsa_device_ab.txt: the smallest auction + finish total that leaves no problem
# capped); that record has not been taken yet, these values come from a numpy model of the algorithm.
EPS_START = 0.1
THETA = 6.0
EPS_FINAL = 1e-4
MAX_ROUNDS = 400000
MAX_COLUMNS = 3584          # csrc/lsa.hip: 44 bytes of LDS per column


def refit_mode():
    if REFIT_LSA not in ("host", "device"):
        raise ValueError("PARSENET_REFIT_LSA must be 'host' or 'device', got %r" % (REFIT_LSA,))
    return REFIT_LSA


def solve_host(cost):
    """Column of every row: scipy on the raw matrix (what the host path and a capped problem run)."""
    return np.asarray(linear_sum_assignment(np.asarray(cost))[1])


def finish_exact(cost, prices):
    """The optimal assignment of ``cost`` (n, m >= n; numpy fp64) from ANY column prices (m,) — the column of every
    row, as ``linear_sum_assignment(cost)[1]``.  The better the prices, the less is left to do."""
    cost = np.asarray(cost, dtype=np.float64)
    if cost.ndim != 2 or cost.shape[0] > cost.shape[1]:
        raise ValueError("finish_exact: cost must be (n, m) with n <= m, got %r" % (cost.shape,))
    n, m = cost.shape
    p = np.asarray(prices, dtype=np.float64).reshape(-1)
    if p.shape[0] != m:
        raise ValueError("finish_exact: %d prices for %d columns" % (p.shape[0], m))
    if not np.isfinite(p).all():
        raise ValueError("finish_exact: non-finite prices")
    if n == 0:
        return np.zeros(0, dtype=np.int64)
    R = np.empty((m, m), dtype=np.float64)
    np.add(cost, p[None, :], out=R[:n])
    R[:n] -= R[:n].min(axis=1, keepdims=True)
    if m > n:
        R[n:] = (p - p.min())[None, :]
    return np.asarray(linear_sum_assignment(R)[1][:n])


def _check_cost(c, what):
    import torch
    if not isinstance(c, torch.Tensor):
        raise ValueError("%s: the cost matrix must be a tensor on the GPU, got %s (the host solver is "
                         "fitting.solve_dense)" % (what, type(c).__name__))
    if c.dtype != torch.float64:
        raise ValueError("%s: the cost matrix must be float64, got %s" % (what, c.dtype))
    if not c.is_cuda:
        raise ValueError("%s: the cost matrix must be on the GPU, got a %s tensor (the host solver is "
                         "fitting.solve_dense)" % (what, c.device))
    if c.dim() != 2 or c.shape[0] < 1 or c.shape[0] > c.shape[1]:
        raise ValueError("%s: the cost matrix must be (n, m) with 1 <= n <= m, got %r" % (what, tuple(c.shape)))
    if c.shape[1] > MAX_COLUMNS:
        raise ValueError("%s: %d columns, the kernel takes at most %d" % (what, c.shape[1], MAX_COLUMNS))


def auction(cost_batch, eps_start=None, theta=None, eps_final=None, max_rounds=None):
    """The auction kernel on a batch: ``cost_batch`` is a list of (n_s, m_s) fp64 GPU tensors (or one (S, n, m)
    tensor); rows may be strided (a view of a wider matrix), columns are contiguous.  ONE launch (per 64 problems).
    Returns a dict of tensors on the device: ``cols`` (S, M) int32 — the column of row i < m_s of the padded square
    problem, -1 beyond or where unassigned —, ``prices`` (S, M) fp64, ``eps`` (S) fp64 the eps reached (absolute),
    ``rounds`` (S) int32, ``status`` (S) int32 (0 complete, 1 stopped by the round cap); M = max m_s."""
    import ctypes

    import torch

    from . import _lib
    costs = list(cost_batch.unbind(0)) if hasattr(cost_batch, "unbind") else list(cost_batch)
    if not costs:
        raise ValueError("auction: an empty batch")
    for c in costs:
        _check_cost(c, "auction")
    dev = costs[0].device
    if any(c.device != dev for c in costs):
        raise ValueError("auction: the cost matrices are on different devices")
    costs = [c if c.stride(1) == 1 and c.stride(0) >= c.shape[1] else c.contiguous() for c in costs]
    S = len(costs)
    M = max(c.shape[1] for c in costs)
    cols = torch.empty((S, M), dtype=torch.int32, device=dev)
    prices = torch.empty((S, M), dtype=torch.float64, device=dev)
    eps = torch.empty(S, dtype=torch.float64, device=dev)
    rounds = torch.empty(S, dtype=torch.int32, device=dev)
    status = torch.empty(S, dtype=torch.int32, device=dev)
    h_cost = (ctypes.c_void_p * S)(*[c.data_ptr() for c in costs])
    h_n = (ctypes.c_int * S)(*[c.shape[0] for c in costs])
    h_m = (ctypes.c_int * S)(*[c.shape[1] for c in costs])
    h_ld = (ctypes.c_int * S)(*[c.stride(0) for c in costs])
    with _lib.on_device(dev):
        rc = _lib.load().pn_lsa_auction_f64(
            ctypes.addressof(h_cost), ctypes.addressof(h_n), ctypes.addressof(h_m), ctypes.addressof(h_ld), S,
            EPS_START if eps_start is None else eps_start, THETA if theta is None else theta,
            EPS_FINAL if eps_final is None else eps_final, MAX_ROUNDS if max_rounds is None else max_rounds, M,
            _lib.ptr(cols), _lib.ptr(prices), _lib.ptr(eps), _lib.ptr(rounds), _lib.ptr(status),
            _lib.current_stream(dev))
    _lib.check(rc, "pn_lsa_auction_f64")
    return {"cols": cols, "prices": prices, "eps": eps, "rounds": rounds, "status": status}


class _DeviceBatch:
    """Cost matrices queued for ONE auction launch.  ``add`` returns a ticket; the first ``cols(ticket)`` launches
    the auction over everything queued, downloads costs and prices and hands the exact finishes to the assignment
    pool (in place without one); a problem the round cap stopped is solved on the host from its raw costs."""

    def __init__(self, **schedule):
        self.costs, self.jobs, self.schedule = [], None, schedule
        self.rounds = self.status = None

    def add(self, cost):
        if self.jobs is not None:
            raise RuntimeError("assignment: this batch has been launched already")
        _check_cost(cost, "assignment")
        self.costs.append(cost)
        return len(self.costs) - 1

    def launch(self):
        from .fitting_eval import assignment_pool
        res = auction(self.costs, **self.schedule)
        prices = res["prices"].cpu().numpy()
        self.status = res["status"].cpu().numpy()
        self.rounds = res["rounds"].cpu().numpy()
        pool = assignment_pool()
        self.jobs = []
        for s, c in enumerate(self.costs):
            cost = c.cpu().numpy()
            if self.status[s] != 0:
                CALLS_LSA["capped"] += 1
                fn, args = solve_host, (cost,)
            else:
                CALLS_LSA["device"] += 1
                fn, args = finish_exact, (cost, prices[s, :cost.shape[1]])
            self.jobs.append(pool.submit(fn, *args) if pool is not None else (fn, args))
        self.costs = None

    def cols(self, ticket):
        if self.jobs is None:
            self.launch()
        job = self.jobs[ticket]
        if isinstance(job, tuple):
            job = self.jobs[ticket] = job[0](*job[1])
        elif hasattr(job, "result"):
            job = self.jobs[ticket] = job.result()
        return job


_QUEUE = None


def queue_device(cost):
    """Queue one cost matrix (fp64, on the GPU) for the next launch -> ``finish()`` returning its columns.  Every
    matrix queued before the first ``finish()`` of any of them goes into the same launch."""
    global _QUEUE
    if _QUEUE is None or _QUEUE.jobs is not None:
        _QUEUE = _DeviceBatch()
    batch, ticket = _QUEUE, _QUEUE.add(cost)
    return lambda: batch.cols(ticket)


def solve_batch_device(costs, **schedule):
    """``costs``: a list of (n_s, m_s) fp64 GPU tensors -> the list of their optimal column arrays (one auction
    launch, the finishes side by side on the assignment pool)."""
    batch = _DeviceBatch(**schedule)
    tickets = [batch.add(c) for c in costs]
    return [batch.cols(t) for t in tickets]


def solve_dense_device(cost, **schedule):
    """``fitting.solve_dense`` for one fp64 cost matrix on the GPU: (rows, cols) of an optimal assignment."""
    _check_cost(cost, "solve_dense_device")
    cols = solve_batch_device([cost], **schedule)[0]
    return np.arange(cols.shape[0]), cols


def refit_submit(dist, host_submit):
    """The matching of one refit segment by the switch: ``dist`` the fp64 distance matrix on the GPU;
    ``host_submit(cost)`` is the caller's own host path (cost downloaded, -> finish()).  Returns finish() -> columns."""
    if refit_mode() == "device":
        return queue_device(dist)
    CALLS_LSA["host"] += 1
    return host_submit(dist.cpu().numpy())
