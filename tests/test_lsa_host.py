"""CPU: the host half of the device assignment path (parsenet_codebase_amd/assignment.py) — the exact finish from
arbitrary column prices against scipy's linear_sum_assignment, the rectangular reduction, the switch."""
import os
import subprocess
import sys

import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (2, 2), (37, 37), (5, 9), (40, 64)]


def _costs(n, m, seed):
    """Distances between random points: continuous, so the optimum is unique."""
    rs = np.random.RandomState(seed)
    a, b = rs.rand(n, 3), rs.rand(m, 3)
    return np.linalg.norm(a[:, None] - b[None], axis=2)


def _prices(c, seed):
    """Zero prices, random prices, and the optimal duals of a DIFFERENT problem of the same shape."""
    n, m = c.shape
    rs = np.random.RandomState(100 + seed)
    other = _costs(m, m, 1000 + seed)
    rows, cols = linear_sum_assignment(other)
    wrong = np.zeros(m)
    wrong[cols] = -other[rows, cols] + other.min(0)[cols] + rs.rand(m)
    return {"zero": np.zeros(m), "random": rs.rand(m) * 3.0 * c.max(), "wrong_problem": wrong - wrong.min()}


@pytest.mark.parametrize("n,m", SHAPES)
def test_finish_exact_from_arbitrary_prices(n, m):
    from parsenet_codebase_amd.assignment import finish_exact
    c = _costs(n, m, n * 131 + m)
    rows, cols = linear_sum_assignment(c)
    want = c[rows, cols].sum()
    for name, p in _prices(c, n + m).items():
        got = finish_exact(c, p)
        assert got.shape == (n,) and len(set(got.tolist())) == n, name
        assert abs(c[np.arange(n), got].sum() - want) <= 1e-12 * abs(want), name
        assert np.array_equal(got, cols), name


@pytest.mark.parametrize("n,m", [(12, 12), (10, 16)])
def test_finish_exact_with_ties_has_the_optimal_cost(n, m):
    """Integer costs in {0..3} with duplicated rows: many optima, the cost is what is pinned."""
    from parsenet_codebase_amd.assignment import finish_exact
    rs = np.random.RandomState(7 + n)
    c = rs.randint(0, 4, (n, m)).astype(np.float64)
    c[1::2] = c[0:-1:2]
    rows, cols = linear_sum_assignment(c)
    want = c[rows, cols].sum()
    for p in (np.zeros(m), rs.rand(m) * 5, rs.randint(0, 3, m).astype(np.float64)):
        got = finish_exact(c, p)
        assert len(set(got.tolist())) == n
        assert abs(c[np.arange(n), got].sum() - want) <= 1e-12 * max(abs(want), 1.0)


def test_rectangular_reduction_is_done_on_the_padded_square():
    """5 x 9 with prices far from optimal: reducing the REAL rows alone and solving that is not optimal (the check
    below shows it on this very case); finish_exact reduces the padded square and is."""
    from parsenet_codebase_amd.assignment import finish_exact
    rs = np.random.RandomState(0)
    c, p = rs.rand(5, 9), rs.rand(9) * 2
    rows, cols = linear_sum_assignment(c)
    want = c[rows, cols].sum()
    naive = c + p
    naive -= naive.min(1, keepdims=True)
    nr, nc = linear_sum_assignment(naive)
    assert c[nr, nc].sum() > want + 0.1                   # the shortcut IS wrong here
    got = finish_exact(c, p)
    assert np.array_equal(got, cols)
    assert abs(c[np.arange(5), got].sum() - want) <= 1e-12 * want


def test_finish_exact_refuses_bad_input():
    from parsenet_codebase_amd.assignment import finish_exact
    with pytest.raises(ValueError, match="n <= m"):
        finish_exact(np.zeros((3, 2)), np.zeros(2))
    with pytest.raises(ValueError, match="prices"):
        finish_exact(np.zeros((2, 3)), np.zeros(2))
    with pytest.raises(ValueError, match="non-finite"):
        finish_exact(np.zeros((2, 2)), np.array([0.0, np.nan]))


def test_switch_defaults_to_host(monkeypatch):
    from parsenet_codebase_amd import assignment
    monkeypatch.delenv("PARSENET_REFIT_LSA", raising=False)
    assert assignment._mode_from_env() == "host"
    monkeypatch.setenv("PARSENET_REFIT_LSA", "device")
    assert assignment._mode_from_env() == "device"
    monkeypatch.setattr(assignment, "REFIT_LSA", "gpu")
    with pytest.raises(ValueError, match="PARSENET_REFIT_LSA"):
        assignment.refit_mode()


def test_host_mode_takes_the_callers_host_path(monkeypatch):
    import torch
    from parsenet_codebase_amd import assignment, fitting_eval
    assert fitting_eval.CALLS_LSA is assignment.CALLS_LSA
    assert set(assignment.CALLS_LSA) == {"device", "host", "capped"}
    monkeypatch.setattr(assignment, "REFIT_LSA", "host")
    before = dict(assignment.CALLS_LSA)
    seen = []

    def host_submit(cost):
        seen.append(cost)
        return lambda: linear_sum_assignment(cost)[1]
    c = _costs(6, 8, 3)
    cols = assignment.refit_submit(torch.from_numpy(c), host_submit)()
    assert len(seen) == 1 and isinstance(seen[0], np.ndarray) and np.array_equal(seen[0], c)
    assert np.array_equal(cols, linear_sum_assignment(c)[1])
    assert assignment.CALLS_LSA["host"] == before["host"] + 1
    assert assignment.CALLS_LSA["device"] == before["device"] and assignment.CALLS_LSA["capped"] == before["capped"]


def test_solve_dense_device_refuses_what_is_not_an_fp64_gpu_tensor():
    import torch
    from parsenet_codebase_amd.assignment import solve_dense_device
    with pytest.raises(ValueError, match="on the GPU"):
        solve_dense_device(torch.zeros(3, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match="float64"):
        solve_dense_device(torch.zeros(3, 3, dtype=torch.float32))
    with pytest.raises(ValueError, match="tensor on the GPU"):
        solve_dense_device(np.zeros((3, 3)))


def test_the_module_a_pool_worker_imports_does_not_import_torch():
    """finish_exact runs in the spawned workers of the assignment pool: importing its module must stay numpy / scipy."""
    code = ("import sys; sys.path.insert(0, %r); import parsenet_codebase_amd.assignment as a; "
            "assert 'torch' not in sys.modules; assert callable(a.finish_exact)" % ROOT)
    subprocess.run([sys.executable, "-c", code], check=True, timeout=120)
