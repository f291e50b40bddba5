"""The opt-in "bf16" arithmetic mode, CPU side: it is selectable (config.set_precision / WF3D_PRECISION), other values
still raise, and its two C entry points (wf3d_gemm_bf16 / wf3d_gemm_bf16_tn) report argument errors without a GPU with
the same codes as the split entry points they mirror.  No kernel is launched here."""
import ctypes
import os
import subprocess
import sys

import pytest

import helpers as H

ERR_ARG, ERR_UNSUPPORTED = -1, -4          # include/wf3d.h: WF3D_ERR_ARG, WF3D_ERR_UNSUPPORTED


def test_set_precision_accepts_bf16_and_restores():
    from wf3d import config
    old = config.precision()
    try:
        config.set_precision("bf16")
        assert config.precision() == "bf16"
        with pytest.raises(ValueError):
            config.set_precision("bf8")
        assert config.precision() == "bf16"
    finally:
        config.set_precision(old)
    assert config.precision() == old


def _import_config(value):
    env = dict(os.environ, WF3D_PRECISION=value)
    code = "import sys; sys.path.insert(0, sys.argv[1]); from wf3d import config; print(config.precision())"
    return subprocess.run([sys.executable, "-c", code, H.PKG], env=env, capture_output=True, text=True, timeout=120)


def test_environment_selects_bf16_in_a_fresh_process():
    r = _import_config("bf16")
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "bf16"


def test_environment_rejects_unknown_precision():
    r = _import_config("bf16x2")
    assert r.returncode != 0
    assert "WF3D_PRECISION" in r.stderr


def test_ops_reject_other_product_counts():
    from wf3d import ops
    with pytest.raises(ValueError):
        ops.gemm_split(None, None, products=2)
    with pytest.raises(ValueError):
        ops.gemm_split_tn(None, None, products=0)


def test_bf16_entry_points_report_argument_errors_without_gpu():
    from wf3d import _lib
    lib = _lib.load()
    # an aligned host buffer stands in for the operands: every call below fails its checks before any launch
    buf = ctypes.create_string_buffer(4096 + 16)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    nt = lib.wf3d_gemm_bf16
    assert nt(p, p, p, None, 4, 4, -1, 8, 8, 4, 0, None, 0, None) == ERR_ARG                    # bad dims
    assert b"wf3d_gemm_bf16" in lib.wf3d_last_error()
    assert nt(p, p, p, None, 4, 4, 12, 16, 16, 4, 0, None, 0, None) == ERR_UNSUPPORTED          # K % 8 != 0
    assert nt(None, p, p, None, 4, 4, 8, 8, 8, 4, 0, None, 0, None) == ERR_ARG                  # null operand
    assert nt(p, p, None, None, 4, 4, 8, 8, 8, 4, 0, None, 0, None) == ERR_ARG
    assert nt(p, p, p, None, 4, 4, 16, 8, 16, 4, 0, None, 0, None) == ERR_ARG                   # lda < K
    assert nt(p, p, p, None, 4, 4, 16, 16, 16, 2, 0, None, 0, None) == ERR_ARG                  # ldc < N
    assert nt(p, p, p, None, 0, 4, 8, 8, 8, 4, 0, None, 0, None) == 0                           # empty: nothing to do
    tn = lib.wf3d_gemm_bf16_tn
    assert tn(p, p, p, 256, 128, 40, 256, 128, 128, 0, None, 0, None) == ERR_UNSUPPORTED        # K % 32 != 0
    assert b"wf3d_gemm_bf16_tn" in lib.wf3d_last_error()
    assert tn(p, p, p, 200, 128, 64, 256, 128, 128, 0, None, 0, None) == ERR_UNSUPPORTED        # Mo % 256 != 0
    assert tn(None, p, p, 256, 128, 64, 256, 128, 128, 0, None, 0, None) == ERR_ARG             # null operand
    assert tn(p, p, p, 256, 128, 64, 128, 128, 128, 0, None, 0, None) == ERR_ARG                # lda < Mo
    assert tn(p, p, p, 256, 128, 64, 256, 128, 64, 0, None, 0, None) == ERR_ARG                 # ldc < No


def test_bf16_entry_points_match_the_split_ones_error_for_error():
    """Same checks in the same order: every argument set gives the split entry point's code."""
    from wf3d import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096 + 16)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    q = ctypes.c_void_p(p.value + 4)                                                             # misaligned
    nt_cases = [(p, p, p, 4, 4, -1, 8, 8, 4), (p, p, p, 4, 4, 12, 16, 16, 4), (None, p, p, 4, 4, 8, 8, 8, 4),
                (p, p, p, 4, 4, 16, 8, 16, 4), (p, p, p, 4, 4, 16, 16, 8, 4), (q, p, p, 4, 4, 8, 8, 8, 4),
                (p, p, p, 4, 4, 8, 12, 8, 4), (p, p, p, -1, 4, 8, 8, 8, 4)]
    for a, b, c, M, N, K, lda, ldb, ldc in nt_cases:
        want = lib.wf3d_gemm_split(a, b, c, None, M, N, K, lda, ldb, ldc, 0, None, 0, None)
        got = lib.wf3d_gemm_bf16(a, b, c, None, M, N, K, lda, ldb, ldc, 0, None, 0, None)
        assert want < 0 and got == want, (M, N, K, lda, ldb, ldc, want, got)
    tn_cases = [(p, p, p, 256, 128, 40, 256, 128, 128), (p, p, p, 256, 64, 64, 256, 128, 128),
                (None, p, p, 256, 128, 64, 256, 128, 128), (p, p, p, 256, 128, 64, 256, 64, 128),
                (q, p, p, 256, 128, 64, 256, 128, 128), (p, p, p, 256, 128, 64, 252, 128, 128)]
    for a, b, c, Mo, No, K, lda, ldb, ldc in tn_cases:
        want = lib.wf3d_gemm_split_tn(a, b, c, Mo, No, K, lda, ldb, ldc, 0, None, 0, None)
        got = lib.wf3d_gemm_bf16_tn(a, b, c, Mo, No, K, lda, ldb, ldc, 0, None, 0, None)
        assert want < 0 and got == want, (Mo, No, K, lda, ldb, ldc, want, got)
