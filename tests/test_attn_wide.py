"""Dispatch of the attention at head widths 64 < hd <= 128 (no GPU needed): these run on the key-tiled MFMA kernels at
every vertex count unless wf3d_set_option("attn_tiled", 0) asks for the VALU kernels, whose LDS check then refuses what
it always refused.  Widths above 128 and below 64 stay on the VALU kernels under every option value."""
import pytest

import helpers as H

WIDE = [(136, 2, 5), (192, 2, 256), (200, 2, 257), (256, 2, 1000), (512, 4, 256), (1024, 8, 64)]
OTHER = [(128, 4, 300), (264, 2, 100), (120, 2, 100)]      # widths 32, 132 and 60


def lib():
    from wf3d import _lib
    return _lib.load()


def defines():
    from wf3d import _lib
    return _lib.DEFINES


def test_wide_head_widths_run_key_tiled_under_the_default_option():
    L = lib()
    for E, heads, vmax in WIDE:
        assert L.wf3d_attn_kernel(E, heads, vmax) == 2, (E, heads, vmax)
    for E, heads, vmax in OTHER:
        assert L.wf3d_attn_kernel(E, heads, vmax) == 0, (E, heads, vmax)


def test_option_0_is_the_valu_arm_and_option_2_moves_nothing_else():
    L = lib()
    with H.lib_option("attn_tiled", 0, default=1):
        for E, heads, vmax in WIDE + OTHER:
            assert L.wf3d_attn_kernel(E, heads, vmax) == 0, (E, heads, vmax)
    with H.lib_option("attn_tiled", 2, default=1):
        for E, heads, vmax in WIDE:
            assert L.wf3d_attn_kernel(E, heads, vmax) == 2, (E, heads, vmax)
        for E, heads, vmax in OTHER:
            assert L.wf3d_attn_kernel(E, heads, vmax) == 0, (E, heads, vmax)
    assert L.wf3d_attn_kernel(256, 2, 1000) == 2                # the default is back


def _null_calls(L, E, heads, vmax=256):
    """wf3d_attn_fwd / wf3d_attn_bwd with every pointer NULL and S = 1: both return before any device call, with the
    LDS refusal (WF3D_ERR_UNSUPPORTED) when it applies and the null-pointer refusal (WF3D_ERR_ARG) otherwise."""
    fwd = L.wf3d_attn_fwd(None, None, 1, vmax, E, heads, 0.0, 0, None, None, None)
    msg_f = L.wf3d_last_error()
    bwd = L.wf3d_attn_bwd(None, None, None, None, None, 1, vmax, E, heads, 0.0, 0, None, None)
    msg_b = L.wf3d_last_error()
    return (fwd, msg_f), (bwd, msg_b)


@pytest.mark.parametrize("option", [1, 2])
def test_width_128_at_256_vertices_is_no_longer_refused(option):
    L, d = lib(), defines()
    with H.lib_option("attn_tiled", option, default=1):
        for rc, msg in _null_calls(L, 256, 2):
            assert rc == d["WF3D_ERR_ARG"] and b"null pointer" in msg, (rc, msg)


def test_width_128_at_256_vertices_is_refused_under_option_0_as_before():
    L, d = lib(), defines()
    with H.lib_option("attn_tiled", 0, default=1):
        for rc, msg in _null_calls(L, 256, 2):
            assert rc == d["WF3D_ERR_UNSUPPORTED"] and b"LDS" in msg, (rc, msg)


@pytest.mark.parametrize("option", [0, 1, 2])
def test_width_264_at_256_vertices_is_still_refused(option):
    L, d = lib(), defines()
    with H.lib_option("attn_tiled", option, default=1):
        for rc, msg in _null_calls(L, 528, 2):
            assert rc == d["WF3D_ERR_UNSUPPORTED"] and b"LDS" in msg, (rc, msg)
