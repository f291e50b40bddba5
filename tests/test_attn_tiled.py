"""Dispatch of the head_dim-64 attention between its kernel families (no GPU needed): wf3d_attn_kernel reports 0 = VALU,
1 = MFMA with the sample resident in LDS, 2 = MFMA key-tiled, under wf3d_set_option("attn_tiled", 0 | 1 | 2)."""
import helpers as H


def test_attn_kernel_follows_the_dispatch_table():
    from wf3d import ops
    assert ops.attn_kernel(512, 8, 256) == 1
    assert ops.attn_kernel(512, 8, 257) == 2
    assert ops.attn_kernel(512, 8, 5) == 1
    assert ops.attn_kernel(128, 4, 300) == 0
    assert ops.attn_kernel(128, 4, 30) == 0
    with H.lib_option("attn_tiled", 0, default=1):
        assert ops.attn_kernel(512, 8, 300) == 0
        assert ops.attn_kernel(512, 8, 256) == 1
    with H.lib_option("attn_tiled", 2, default=1):
        assert ops.attn_kernel(512, 8, 5) == 2
        assert ops.attn_kernel(512, 8, 1000) == 2
        assert ops.attn_kernel(128, 4, 300) == 0            # other head widths stay on the VALU kernels
    assert ops.attn_kernel(512, 8, 257) == 2                # the default is back


def test_attn_tiled_option_validates():
    from wf3d import _lib
    lib = _lib.load()
    try:
        for v in (0, 2, 1):
            assert lib.wf3d_set_option(b"attn_tiled", v) == 0
        for v in (3, -1):
            assert lib.wf3d_set_option(b"attn_tiled", v) == -1 and b"attn_tiled" in lib.wf3d_last_error()
        assert lib.wf3d_attn_kernel(512, 8, 300) == 2       # a refused value changes nothing
        assert lib.wf3d_attn_kernel(512, 0, 300) == -1 and lib.wf3d_attn_kernel(512, 7, 300) == -1
    finally:
        assert lib.wf3d_set_option(b"attn_tiled", 1) == 0
