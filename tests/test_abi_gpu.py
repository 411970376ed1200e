"""The two entry points that write through HOST pointers, pn_prof_get and pn_meanshift_x3_exec_tiles: the ctypes
table derived from include/parsenet_hip.h types every pointer as c_void_p, and _lib.prof_results() /
_lib.meanshift_exec_tiles() hand them ctypes.byref(...), a string buffer and a ctypes array."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu


def test_profiler_and_tile_counters_through_the_derived_table(gpu):
    from parsenet_codebase_amd import _lib, kernels as K
    torch.cuda.set_device(gpu)
    g = torch.Generator().manual_seed(0)
    a, b = torch.rand(1, 64, 3, generator=g).to(gpu), torch.rand(1, 64, 3, generator=g).to(gpu)
    # B = 1, N = 1: pn_meanshift_x3_iter_fwd_kind_f32 refuses only B <= 0 or N <= 0 (one row, one padded tile pair)
    x = torch.nn.functional.normalize(torch.randn(1, 1, 128, generator=g), dim=2).to(gpu)
    bsq = torch.full((1,), 0.09, device=gpu)
    img, ws = K.meanshift_x3_split(x), K.MeanShiftWorkspace(1, 1, 128, gpu)
    _lib.meanshift_exec_tiles()                     # what earlier launches of this process counted
    _lib.prof_reset()
    _lib.prof_enable(True)
    try:
        K.chamfer_nn(a, b)
        K.meanshift_x3_iter_fwd(x, img, bsq, ws)
        families = _lib.prof_results()
    finally:
        _lib.prof_enable(False)
        _lib.prof_reset()
    chamfer = {k: v for k, v in families.items() if k.startswith("chamfer")}
    assert chamfer, families
    for ms, calls in chamfer.values():
        assert isinstance(calls, int) and calls >= 1 and math.isfinite(ms) and ms >= 0.0
    ms, calls = families["meanshift_fwd"]
    assert calls >= 1 and math.isfinite(ms) and ms >= 0.0
    tiles = _lib.meanshift_exec_tiles()
    assert len(tiles) == 3 and all(isinstance(t, int) and t >= 0 for t in tiles) and tiles[0] > 0
    assert _lib.meanshift_exec_tiles() == (0, 0, 0)
