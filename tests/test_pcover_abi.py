"""CPU-side checks of the point coverage of the fitted primitives (p-coverage): the export of csrc/cover.hip and ABI
23, the header / ctypes table, the drop-in module src.eval_utils, the value-only residual of csrc/fit_math.h compiled
for the host against the fixture the reference wrote (tests/golden/make_golden_pcover.py), and the argument checks of
metrics.p_coverage that need no GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "parsenet_hip.h")
NAMES = ["pn_point_primitive_min_f32", "pn_point_primitive_min_tile"]
KINDS = {"plane": 0, "sphere": 1, "cylinder": 2, "cone": 3}


@pytest.fixture(scope="module")
def lib_path():
    from parsenet_codebase_amd import build
    return build.build(verbose=False)


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(ROOT, "tests", "golden", "pcover.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cvh") / "libcvh.so")
    src = os.path.join(ROOT, "tests", "native", "cover_math_host.cpp")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", out, src], check=True)
    return ctypes.CDLL(out)


def test_library_exports_the_entry_point_at_abi_23(lib_path):
    lib = ctypes.CDLL(lib_path)
    assert all(hasattr(lib, n) for n in NAMES)
    lib.pn_abi_version.restype = ctypes.c_int
    assert lib.pn_abi_version() == 23
    lib.pn_point_primitive_min_tile.restype = ctypes.c_int
    assert lib.pn_point_primitive_min_tile() % 64 == 0


def test_header_and_ctypes_table_agree(lib_path):
    from parsenet_codebase_amd import _lib
    assert _lib.ABI_VERSION == 23
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NAMES:
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, txt)
        assert m, name
        args = [a for a in m.group(1).split(",") if a.strip() not in ("", "void")]
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(args), name


def test_eval_utils_names_are_the_packages():
    import src.eval_utils as E
    from parsenet_codebase_amd import fitting, metrics
    for name in ("p_coverage", "mean_IOU_one_sample", "iou_segmentation", "matching_iou", "relaxed_iou",
                 "separate_losses"):
        assert getattr(E, name) is getattr(metrics, name), name
    assert E.to_one_hot is fitting.to_one_hot
    assert not any(hasattr(E, n) for n in ("IOU", "IOU_simple", "preprocess"))
    assert callable(fitting.Evaluation.p_coverage)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_value_only_residual_reproduces_the_reference(harness, fx, kind):
    """residual_point_value (host build) on every point of the three fixture shapes against the reference's
    per-primitive fp32 distances, within 4 x the reference's own fp32 error for the type; and bit for bit the value
    of the dual-number residual_point it restates."""
    th = np.zeros(16, np.float32)
    flat = np.concatenate([fx["%s_p%d" % (kind, i)].reshape(-1) for i in range(3 if kind in ("cylinder", "cone") else 2)])
    th[:flat.shape[0]] = flat
    bar = 4.0 * float(fx["noise"][list(fx["types"]).index(kind)])
    assert 0 < bar < 1e-5
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    seen = 0
    for tag in "abc":
        rows = [s for s, n in enumerate(x for x in fx[tag + "_names"] if x != "none") if n == kind]
        if not rows:
            continue
        pts = np.ascontiguousarray(fx[tag + "_points"], np.float32)
        val, dual = np.zeros(pts.shape[0], np.float32), np.zeros(pts.shape[0], np.float32)
        harness.cvh_residuals(p(pts), pts.shape[0], KINDS[kind], p(th), 1, p(val), p(dual))
        assert np.array_equal(val, dual)
        for s in rows:
            err = np.abs(val.astype(np.float64) - fx[tag + "_d32"][s].astype(np.float64)).max()
            print("%s shape %s row %d: max |host - reference fp32| = %.3e, bar %.3e" % (kind, tag, s, err, bar))
            assert err <= bar
            seen += 1
    assert seen >= 2


def test_no_fitted_primitive_is_a_value_error():
    from parsenet_codebase_amd import metrics
    pts = np.zeros((8, 3), np.float32)
    for prm in ({}, {0: None, 3: None}):
        with pytest.raises(ValueError, match="no fitted primitive"):
            metrics.p_coverage(pts, prm)
        with pytest.raises(ValueError, match="no fitted primitive"):
            metrics.p_coverage_batch([pts], [prm])


def test_unknown_switch_value_names_the_two_paths(monkeypatch):
    from parsenet_codebase_amd import metrics
    assert metrics.DEFAULT_PCOVER in metrics.CALLS_PCOVER and sorted(metrics.CALLS_PCOVER) == ["fused", "tensor"]
    monkeypatch.setenv("PARSENET_PCOVER", "bogus")
    with pytest.raises(ValueError, match="fused.*tensor"):
        metrics.p_coverage(np.zeros((8, 3), np.float32), {0: ["plane", np.zeros((3, 1), np.float32), 0.0]})


def test_separate_losses_skips_small_segments_and_none_entries():
    """src.eval_utils.separate_losses (eval_utils.py:130-175): segments with fewer than 100 ground-truth points and
    None entries do not count; a residual above 1 is replaced by 0.1; splines are weighted by lamb."""
    import torch
    import src.eval_utils as E
    gt = {0: np.zeros((150, 3)), 1: np.zeros((99, 3)), 2: None, 3: np.zeros((100, 3)), 4: np.zeros((120, 3))}
    dist = {0: ["plane", torch.tensor(0.25)], 1: ["sphere", torch.tensor(0.5)], 2: ["cone", torch.tensor(0.75)],
            3: ["open-spline", torch.tensor(0.125)], 4: ["cylinder", torch.tensor(2.0)]}
    loss, geometric, spline = E.separate_losses(dist, gt, lamb=2.0)
    assert geometric == pytest.approx((0.25 + 0.1) / 2) and spline == pytest.approx(0.125)
    assert loss.item() == pytest.approx((0.25 + 2.0 * 0.125 + 0.1) / 3)
    assert dist[4][1].item() == pytest.approx(0.1) and dist[1][1].item() == 0.5      # the skipped one is untouched
