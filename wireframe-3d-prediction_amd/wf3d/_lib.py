"""ctypes binding of libwf3d.so (C ABI: include/wf3d.h).

The HIP library is the product path.  There is NO fallback: if the shared
object is missing or a symbol is absent, importing this module raises.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("WF3D_LIB", os.path.join(os.path.dirname(_HERE), "libwf3d.so"))   # override: timing-only ablation builds

c_float_p = ctypes.c_void_p      # device pointers travel as plain addresses
c_void_p = ctypes.c_void_p
c_int = ctypes.c_int
c_size_t = ctypes.c_size_t
c_float = ctypes.c_float
c_u32 = ctypes.c_uint32


class GemmDesc(ctypes.Structure):
    """Mirror of `wf3d_gemm_t` (include/wf3d.h)."""
    _fields_ = [
        ("A", c_void_p), ("B", c_void_p), ("C", c_void_p),
        ("bias", c_void_p), ("addend", c_void_p),
        ("M", c_int), ("N", c_int), ("K", c_int),
        ("lda", c_int), ("ldb", c_int), ("ldc", c_int), ("ld_addend", c_int),
        ("layout", c_int), ("pro_act", c_int), ("pro_enable", c_int),
        ("pro_mu", c_void_p), ("pro_rs", c_void_p), ("pro_gamma", c_void_p), ("pro_beta", c_void_p),
        ("drop_p", c_float), ("drop_seed", c_u32),
        ("accumulate", c_int),
        ("ws", c_void_p), ("ws_bytes", c_size_t),
        ("x3", c_int),
        ("lr_u", c_void_p), ("lr_v", c_void_p), ("lr_k", c_int), ("ld_lr_u", c_int), ("ld_lr_v", c_int),
    ]


class SkinnyFwd(ctypes.Structure):
    """Mirror of `wf3d_skinny_fwd_t`."""
    _fields_ = [
        ("X", c_void_p), ("ldx", c_int), ("W", c_void_p), ("ldw", c_int), ("bias", c_void_p),
        ("Y", c_void_p), ("ldy", c_int), ("N", c_int), ("K", c_int),
        ("gamma", c_void_p), ("beta", c_void_p), ("act", c_int),
        ("in_part", c_void_p), ("in_nblk", c_int), ("mu", c_void_p), ("rs", c_void_p),
        ("mu_out", c_void_p), ("rs_out", c_void_p),
        ("in_addend", c_void_p), ("ld_in_addend", c_int),
        ("out_addend", c_void_p), ("ld_out_addend", c_int),
        ("stat_part", c_void_p),
    ]


class SkinnyBwd(ctypes.Structure):
    """Mirror of `wf3d_skinny_bwd_t`."""
    _fields_ = [
        ("dY", c_void_p), ("lddy", c_int),
        ("z", c_void_p), ("ldz", c_int), ("mu", c_void_p), ("rs", c_void_p), ("rowpart", c_void_p), ("rowpart_nblk", c_int),
        ("W", c_void_p), ("ldw", c_int), ("N", c_int), ("K", c_int),
        ("X", c_void_p), ("ldx", c_int),
        ("xmu", c_void_p), ("xrs", c_void_p), ("xgamma", c_void_p), ("xbeta", c_void_p), ("xact", c_int),
        ("xadd", c_void_p), ("ldxadd", c_int),
        ("dW", c_void_p), ("lddw", c_int), ("db", c_void_p),
        ("slabs", c_void_p), ("nc", c_int),
    ]


class SkinnyRed(ctypes.Structure):
    """Mirror of `wf3d_skinny_red_t`."""
    _fields_ = [
        ("slabs", c_void_p * 3), ("nslab", c_int * 3),
        ("extra", c_void_p), ("ldextra", c_int), ("K", c_int),
        ("dh", c_void_p), ("lddh", c_int),
        ("z", c_void_p), ("ldz", c_int), ("mu", c_void_p), ("rs", c_void_p), ("gamma", c_void_p), ("beta", c_void_p),
        ("act", c_int),
        ("G", c_void_p), ("ldg", c_int), ("dgamma", c_void_p), ("dbeta", c_void_p), ("rowpart", c_void_p),
    ]


# name -> (restype, argtypes); every symbol include/wf3d.h declares
SIGNATURES = {
    "wf3d_version": (c_int, []),
    "wf3d_last_error": (ctypes.c_char_p, []),
    "wf3d_set_option": (c_int, [ctypes.c_char_p, c_int]),
    "wf3d_gemm_ws_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "wf3d_gemm": (c_int, [ctypes.POINTER(GemmDesc), c_void_p]),
    "wf3d_row_stats": (c_int, [c_void_p, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p]),
    "wf3d_ln_act_apply": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                  c_void_p, c_float, c_u32, c_void_p, c_void_p]),
    "wf3d_ln_act_bwd_ws_bytes": (c_size_t, [c_int, c_int]),
    "wf3d_ln_act_bwd": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                c_float, c_u32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                c_void_p]),
    "wf3d_gemm_split_ws_bytes": (c_size_t, [c_int, c_int, c_int]),
    "wf3d_gemm_split": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                                c_int, c_void_p, c_size_t, c_void_p]),
    "wf3d_gemm_split_tn_ok": (c_int, [c_int, c_int, c_int, c_int, c_int]),
    "wf3d_gemm_split_tn_ws_bytes": (c_size_t, [c_int, c_int, c_int]),
    "wf3d_gemm_split_tn": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                   c_void_p, c_size_t, c_void_p]),
    "wf3d_gemm_bf16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                               c_int, c_void_p, c_size_t, c_void_p]),
    "wf3d_gemm_bf16_tn": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                  c_void_p, c_size_t, c_void_p]),
    "wf3d_split_rows": (c_int, [c_void_p, ctypes.c_long, ctypes.c_long, c_int, c_int, c_void_p, c_void_p]),
    "wf3d_split_rows_multi": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "wf3d_split_transpose": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                     c_float, c_u32, c_int, c_void_p, c_void_p]),
    "wf3d_ln_prep": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_float, c_float, c_u32, c_void_p,
                             c_void_p, c_void_p, c_void_p]),
    "wf3d_colsum_ws_bytes": (c_size_t, [c_int, c_int]),
    "wf3d_colsum": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "wf3d_point_valid": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "wf3d_pool4_ws_bytes": (c_size_t, [c_int, c_int, c_int]),
    "wf3d_pool4_fwd": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                               c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "wf3d_pool4_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                               c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "wf3d_pool4_bwd_bias": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                    c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "wf3d_first_layer_fwd": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p,
                                     c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "wf3d_ln_act_bwd_first_ws_bytes": (c_size_t, [c_int, c_int]),
    "wf3d_ln_act_bwd_first": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_size_t, c_void_p]),
    "wf3d_ln_act_bwd_wsum_ws_bytes": (c_size_t, [c_int, c_int]),
    "wf3d_ln_act_bwd_wsum": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_int, c_float, ctypes.c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_size_t, c_void_p]),
    "wf3d_rowdot_act_ok": (c_int, [c_int]),
    "wf3d_rowdot_act": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "wf3d_rowdot_act_bwd_ws_bytes": (c_size_t, [c_int, c_int]),
    "wf3d_rowdot_act_bwd": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                    c_void_p, c_void_p, c_size_t, c_void_p]),
    "wf3d_pool4_bwd_sx8": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                   c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "wf3d_pool4_seg_ws_bytes": (c_size_t, [c_int, c_int]),
    "wf3d_pool4_seg_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p,
                                   c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_size_t, c_void_p]),
    "wf3d_pool4_seg_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                   c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p,
                                   c_void_p]),
    "wf3d_pool4_seg_bwd_sx8": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                       c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                                       c_void_p, c_void_p]),
    "wf3d_packed_layout_dims": (c_int, [c_int, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    "wf3d_packed_layout_build": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "wf3d_packed_layout_build_i32": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "wf3d_vertex_finalize_fwd": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "wf3d_vertex_finalize_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "wf3d_edge_layout": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_void_p]),
    "wf3d_edge_gather_verts": (c_int, [c_void_p, ctypes.c_long, ctypes.c_long, c_void_p, c_void_p, c_int, c_int, c_void_p,
                                       c_void_p]),
    "wf3d_edge_scatter_dverts": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "wf3d_attn_fwd": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_u32, c_void_p, c_void_p,
                              c_void_p]),
    "wf3d_attn_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float,
                              c_u32, c_void_p, c_void_p]),
    "wf3d_attn_kernel": (c_int, [c_int, c_int, c_int]),
    "wf3d_edge_pair_ln_bwd_ws_bytes": (c_size_t, [c_int, c_int]),
    "wf3d_edge_pair_ln_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int,
                                      c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_float, c_u32, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "wf3d_edge_pair_fwd_ln": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                      c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_float,
                                      ctypes.c_uint32, c_void_p, c_void_p]),
    "wf3d_edge_pair_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                   c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "wf3d_edge_pair_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                   c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "wf3d_edge_prob_fwd": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "wf3d_loss_cost_matrix": (c_int, [c_void_p, ctypes.c_long, ctypes.c_long, c_void_p, c_void_p, c_int, c_void_p, c_int,
                                      c_int, c_void_p, c_void_p]),
    "wf3d_loss_assign": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "wf3d_loss_assign_counts": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "wf3d_loss_terms_assigned": (c_int, [c_void_p, ctypes.c_long, ctypes.c_long, c_void_p, c_void_p, c_int, c_void_p,
                                         c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_float,
                                         c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                         c_void_p]),
    "wf3d_loss_terms_assigned_ew": (c_int, [c_void_p, ctypes.c_long, ctypes.c_long, c_void_p, c_void_p, c_int, c_void_p,
                                            c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                            c_float, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                            c_size_t, c_void_p]),
    "wf3d_loss_terms": (c_int, [c_void_p, ctypes.c_long, ctypes.c_long, c_void_p, c_void_p, c_int, c_void_p, c_int,
                                c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float,
                                c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                c_void_p]),
    "wf3d_skinny_ok": (c_int, [c_int, c_int]),
    "wf3d_skinny_fwd": (c_int, [ctypes.POINTER(SkinnyFwd), c_int, c_int, c_float, c_void_p]),
    "wf3d_skinny_slab_floats": (c_size_t, [c_int, c_int, c_int, c_int]),
    "wf3d_skinny_bwd": (c_int, [ctypes.POINTER(SkinnyBwd), c_int, c_int, c_void_p]),
    "wf3d_skinny_reduce": (c_int, [ctypes.POINTER(SkinnyRed), c_int, c_void_p]),
    "wf3d_clip_adam_ws_floats": (c_size_t, [c_void_p, c_int]),
    "wf3d_clip_adam_step": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, ctypes.c_double, ctypes.c_double,
                                    ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, c_int, c_void_p,
                                    c_size_t, c_void_p, c_void_p]),
    "wf3d_clip_adam_step_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, ctypes.c_double,
                                        ctypes.c_double, c_void_p, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                        ctypes.c_double, c_void_p, c_size_t, c_void_p, c_void_p]),
    "wf3d_dropout_draw": (c_int, [c_void_p, c_void_p, c_void_p]),
    "wf3d_set_dropout_seed_words": (c_int, [c_void_p]),
    "wf3d_set_live_rows": (c_int, [c_void_p]),
    "wf3d_cloud_normalize": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "wf3d_cloud_sample": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "wf3d_meter_update": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_long, c_void_p, ctypes.c_long, c_void_p,
                                  c_int, c_void_p, c_int, c_void_p]),
    "wf3d_parse_floats": (ctypes.c_long, [ctypes.c_char_p, c_void_p, ctypes.c_long]),
    "wf3d_parse_table": (ctypes.c_long, [ctypes.c_char_p, c_void_p, ctypes.c_long, ctypes.POINTER(ctypes.c_long)]),
    "wf3d_edge_endpoints": (c_int, [c_void_p, ctypes.c_long, ctypes.c_long, c_void_p, c_void_p, c_int, c_int, c_int, c_float,
                                    c_void_p, c_void_p, c_void_p]),
    "wf3d_hausdorff_lines": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "wf3d_edge_prob_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
}

_lib = None


def load():
    """Load libwf3d.so once.  torch must be imported first so that the HIP
    runtime torch bundles (same soname, libamdhip64.so.7) is the one in the
    process; ours then binds to it instead of loading a second runtime."""
    global _lib
    if _lib is not None:
        return _lib
    import torch  # noqa: F401  (see docstring)
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"wf3d: {LIB_PATH} not found — the HIP extension is required (no CPU fallback). "
            "Build it with `python -c 'import __graft_entry__ as g; g.build()'` or "
            "`make -C wireframe-3d-prediction_amd/csrc`.")
    lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_LOCAL)
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise RuntimeError(f"wf3d: libwf3d.so lacks symbol {name}; rebuild it") from e
        fn.restype = res
        fn.argtypes = args
    if lib.wf3d_version() < 102:
        raise RuntimeError("wf3d: libwf3d.so is stale; rebuild it")
    _lib = lib
    try:
        set_tn_rounds(1)
    except Exception:
        _lib = None
        raise
    return lib


def set_tn_rounds(default):
    """wf3d_set_option("tn_rounds", n): workgroups per CU of the large weight-gradient launches (include/wf3d.h).
    n = $WF3D_TN_ROUNDS when set, else `default`: 1 from load(), 2 from wf3d.dist.GradReducer across ranks."""
    v = os.environ.get("WF3D_TN_ROUNDS")
    n = int(v) if v else default
    if not 1 <= n <= 8:
        raise ValueError(f"wf3d: WF3D_TN_ROUNDS must be 1..8 (got {v!r})")
    check(load().wf3d_set_option(b"tn_rounds", n), "wf3d_set_option(tn_rounds)")


def check(code, what):
    if code != 0:
        msg = load().wf3d_last_error().decode(errors="replace")
        raise RuntimeError(f"wf3d: {what} failed (code {code}): {msg}")
