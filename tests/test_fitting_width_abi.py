"""CPU: what the entry points behind the batched fitting stage and the embedding loss can show without a device.
The row-restricted mean-shift backward (csrc/meanshift_rows.hip), the membership kernels and the triplet kernels
(csrc/fused.hip) are instantiated at widths 32, 64 and 128: every other width is refused before anything is
launched, with a message that names the supported set — never served by something else."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from parsenet_codebase_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def _refused(lib, rc, who):
    msg = lib.pn_last_error().decode("utf-8", "replace")
    assert rc != 0, who
    assert who in msg and "{32, 64, 128}" in msg, msg
    return msg


def test_width_48_is_refused_with_the_supported_set(lib):
    # host buffers stand in for device pointers: the width check comes before any launch and nothing reads them
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    D = 48
    rc = lib.pn_meanshift_rows_bwd_f32(p, p, p, p, p, p, p, 1, 100, D, 4, p, p, p, 1 << 30, None)
    assert "48" in _refused(lib, rc, "pn_meanshift_rows_bwd_f32")
    rc = lib.pn_meanshift_rows_scatter_add_f32(p, p, 1, 100, D, 4, p, None)
    _refused(lib, rc, "pn_meanshift_rows_scatter_add_f32")
    rc = lib.pn_membership_fwd_f32(p, p, p, p, 1, 16, 100, D, 1e-7, p, p, p, p, p, None)
    assert rc == -4 and "D=48" in _refused(lib, rc, "pn_membership_fwd_f32")
    rc = lib.pn_triplet_fwd_f32(p, 100, D, p, p, p, 2, 8, 1.0, p, p, p, None)
    assert rc == -4 and "48" in _refused(lib, rc, "pn_triplet_fwd_f32")
    rc = lib.pn_triplet_bwd_f32(p, 100, D, p, p, p, p, 2, 8, 1.0, p, p, 1 << 30, None)
    assert rc == -4 and "48" in _refused(lib, rc, "pn_triplet_bwd_f32")


def test_row_backward_workspace_does_not_depend_on_the_width(lib):
    """pn_meanshift_rows_bwd_workspace(B, N) has no D: it is sized for the widest instantiation — what the
    128-wide path asked for before — and grows with the number of 64-point column blocks."""
    B, N = 4, 10000
    nblk = (N + 63) // 64
    want = B * nblk * 64 * 128 * 4 + B * 64 * 128 * 4 + B * 64 * 4 * 4
    assert lib.pn_meanshift_rows_bwd_workspace(B, N) == want
    assert lib.pn_meanshift_rows_bwd_workspace(B, 64) < lib.pn_meanshift_rows_bwd_workspace(B, 65)
    # the triplet backward's slots shrink with the width
    assert lib.pn_triplet_bwd_workspace(10, 30, 32) * 4 == lib.pn_triplet_bwd_workspace(10, 30, 128)


def test_padding_widths_of_the_python_layers():
    from parsenet_codebase_amd import fitting_batch as FB, losses
    assert [losses.triplet_width(d) for d in (1, 32, 33, 50, 64, 65, 128, 129)] == [32, 32, 64, 64, 64, 128, 128, None]
    assert FB.MEMBERSHIP_WIDTHS == (32, 64, 128)
    assert FB.CALLS_STAGE.keys() == {"batched", "per_shape"} and isinstance(losses.CALLS_TRIPLET_FUSED, int)
