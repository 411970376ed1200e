"""CPU-side checks of what the raw-cloud kernels share: ``ragged.Clouds`` (pure shape logic, built here from CPU
tensors with the device check skipped), csrc/ragged.h through its stand-alone program (tests/native/ragged_host.cpp),
and the three workspace sizes held to the values recorded before the carver replaced the hand-written sums
(tests/golden/ragged_workspace_bytes.json)."""
import itertools
import json
import os
import subprocess

import numpy as np
import pytest
import torch

from parsenet_codebase_amd.ragged import Clouds
from tests.helpers import native

LAYOUTS = ("single", "batch", "list")
TRAILING = ((), (4,), (2, 3))


def clouds_of(layout, sizes=(0, 1, 5), seed=0):
    """(points in the layout, Clouds, the clouds as a list of (n,3) tensors)."""
    g = torch.Generator().manual_seed(seed)
    if layout == "single":
        parts = [torch.rand((7, 3), generator=g)]
        points = parts[0]
    elif layout == "batch":
        points = torch.rand((3, 4, 3), generator=g)
        parts = list(points)
    else:
        parts = [torch.rand((n, 3), generator=g) for n in sizes]
        points = parts
    return points, Clouds(points, "test", on_gpu=False), parts


def as_list(layout, value):
    """A value in a layout as the list of its per-cloud tensors."""
    return [value] if layout == "single" else list(value)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_flat_view_and_the_offsets(layout):
    points, c, parts = clouds_of(layout)
    sizes = [p.shape[0] for p in parts]
    assert c.sizes == sizes and c.S == len(parts) and c.total == sum(sizes) and c.max_n == max(sizes)
    assert c.layout == {"single": "single", "list": "list", "batch": (3, 4)}[layout]
    assert c.off.dtype == np.int64 and c.off.tolist() == [0] + np.cumsum(sizes).tolist()
    assert torch.equal(c.flat, torch.cat(parts)) and tuple(c.flat.shape) == (c.total, 3)
    for s, p in enumerate(parts):
        assert torch.equal(c.flat[c.off[s]:c.off[s + 1]], p)


@pytest.mark.parametrize("sizes", sorted(set(itertools.permutations((0, 1, 5)))))
def test_an_empty_cloud_first_in_the_middle_and_last(sizes):
    _, c, parts = clouds_of("list", sizes)
    assert c.sizes == list(sizes) and c.off.tolist() == [0] + np.cumsum(sizes).tolist() and c.max_n == 5
    labels = torch.arange(c.total)
    back = c.per_point(labels)
    assert [tuple(b.shape) for b in back] == [(n,) for n in sizes]
    assert torch.equal(torch.cat(back), labels) and torch.equal(c.beside(back, "test", "labels"), labels)
    rows = torch.arange(3 * 2).reshape(3, 2)
    assert all(torch.equal(r, rows[s]) for s, r in enumerate(c.per_cloud(rows)))


@pytest.mark.parametrize("trailing", TRAILING)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_per_point_results_round_trip(layout, trailing):
    _, c, parts = clouds_of(layout)
    flat = torch.arange(c.total * int(np.prod(trailing, dtype=np.int64))).reshape((c.total,) + trailing)
    shaped = c.per_point(flat)
    pieces = as_list(layout, shaped)
    assert isinstance(shaped, list) == (layout == "list")
    assert [tuple(p.shape) for p in pieces] == [(n,) + trailing for n in c.sizes]
    for s, p in enumerate(pieces):
        assert torch.equal(p, flat[c.off[s]:c.off[s + 1]])
    if layout == "batch":
        assert tuple(shaped.shape) == (3, 4) + trailing
    # and back: the result of a call is a valid companion of its points
    assert torch.equal(c.beside(shaped, "test", "values"), flat)


@pytest.mark.parametrize("trailing", TRAILING)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_per_cloud_rows(layout, trailing):
    _, c, _ = clouds_of(layout)
    m = 2
    rows = torch.arange(c.S * m * int(np.prod(trailing, dtype=np.int64))).reshape((c.S, m) + trailing)
    shaped = c.per_cloud(rows)
    assert isinstance(shaped, list) == (layout == "list")
    if layout == "single":
        assert tuple(shaped.shape) == (m,) + trailing and torch.equal(shaped, rows[0])
    else:
        assert len(shaped) == c.S and all(torch.equal(a, b) for a, b in zip(shaped, rows))


def test_an_empty_batch():
    """(0,N,3): no cloud at all.  estimate_normals and orient_normals give an empty (0,N,...) result on it."""
    c = Clouds(torch.zeros(0, 5, 3), "test", on_gpu=False)
    assert c.layout == (0, 5) and c.sizes == [] and (c.S, c.total, c.max_n) == (0, 0, 0) and c.off.tolist() == [0]
    assert tuple(c.flat.shape) == (0, 3)
    assert tuple(c.per_point(torch.zeros(0, 3)).shape) == (0, 5, 3) and tuple(c.per_point(torch.zeros(0)).shape) == (0, 5)
    assert tuple(c.per_cloud(torch.zeros(0, 2, 3)).shape) == (0, 2, 3)
    assert tuple(c.beside(torch.zeros(0, 5, 4), "test", "values").shape) == (0, 4)
    with pytest.raises(ValueError, match="same layout"):
        c.beside(torch.zeros(0, 4, 3), "test", "values")


def test_a_companion_in_another_layout_or_size_is_refused():
    _, single, _ = clouds_of("single")
    _, batch, _ = clouds_of("batch")
    _, ragged, parts = clouds_of("list")
    wrong = [
        (single, torch.zeros(8, 3)),                                     # another size
        (single, [torch.zeros(7, 3)]),                                   # a list against a single cloud
        (single, torch.zeros(())),
        (batch, torch.zeros(3, 5, 3)),                                   # another N
        (batch, torch.zeros(12, 3)),                                     # flat against a batch
        (batch, [torch.zeros(4, 3)] * 3),                                # a list against a batch
        (ragged, torch.zeros(6, 3)),                                     # a tensor against a list
        (ragged, [torch.zeros(0, 3), torch.zeros(1, 3)]),                # too few
        (ragged, [torch.zeros(1, 3), torch.zeros(0, 3), torch.zeros(5, 3)]),      # the sizes in another order
        (ragged, []),
    ]
    for c, array in wrong:
        with pytest.raises(ValueError, match="test: normals must have the same layout and sizes"):
            c.beside(array, "test", "normals")
    for array in (np.zeros((7, 3)), None, [np.zeros((7, 3))]):
        with pytest.raises(TypeError, match="normals must be a tensor or a list of tensors"):
            single.beside(array, "test", "normals")
    assert ragged.beside([torch.zeros(n, dtype=torch.int64) for n in ragged.sizes], "test", "labels").dtype == torch.int64


def test_the_errors_of_the_constructor():
    with pytest.raises(ValueError, match="empty list"):
        Clouds([], "test", on_gpu=False)
    with pytest.raises(TypeError, match="holds tensors"):
        Clouds([torch.zeros(3, 3), np.zeros((3, 3))], "test", on_gpu=False)
    with pytest.raises(TypeError, match="tensor or a list"):
        Clouds(np.zeros((3, 3)), "test", on_gpu=False)
    for bad in (torch.zeros(3, 4), torch.zeros(3), torch.zeros(2, 2, 3, 3), [torch.zeros(2, 3, 3)]):
        with pytest.raises(ValueError, match=r"\(N,3\)"):
            Clouds(bad, "test", on_gpu=False)
    with pytest.raises(ValueError, match="float32"):
        Clouds(torch.zeros(3, 3, dtype=torch.float64), "test", on_gpu=False)
    with pytest.raises(TypeError, match="float32"):
        Clouds(torch.zeros(3, 3, dtype=torch.float64), "test", bad_dtype=TypeError, on_gpu=False)
    with pytest.raises(RuntimeError, match="MI355X only"):
        Clouds(torch.zeros(3, 3), "test")
    with pytest.raises(RuntimeError, match="MI355X only"):                  # the device before the layout
        Clouds(torch.zeros(3, 4, dtype=torch.float64), "test")


def test_the_header_checks_itself(tmp_path):
    """csrc/ragged.h for the host: the search against a linear scan on every small offsets vector under both keys, the
    predicates against their definitions, the carver's two passes."""
    exe = native.build_program(tmp_path, "ragged_host", native.source("ragged_host.cpp"))
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("ragged_host: 5461 offsets vectors; differences: search 0, predicates 0, carver 0")


def test_the_workspace_sizes_are_those_of_the_hand_written_sums():
    lib = native.load_raw(("pn_knn3_grid_workspace_bytes", "pn_orient_normals_global_workspace_bytes",
                           "pn_fps_workspace_bytes"))
    with open(os.path.join(native.ROOT, "tests", "golden", "ragged_workspace_bytes.json")) as f:
        table = json.load(f)
    assert sorted(table) == ["pn_fps_workspace_bytes", "pn_knn3_grid_workspace_bytes",
                             "pn_orient_normals_global_workspace_bytes"]
    for name, rows in table.items():
        assert len(rows) >= 28
        for *args, want in rows:
            assert getattr(lib, name)(*args) == want, (name, args)
        assert any(want == 0 for *_, want in rows) and any(want > 2 ** 32 for *_, want in rows)
