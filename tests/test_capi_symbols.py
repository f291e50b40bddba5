"""CPU-side checks of the drop-in boundary: libwf3d.so loads without a GPU and
exports every symbol include/wf3d.h declares, with the argument checks of the
C ABI reachable (no kernel is launched here)."""
import ctypes
import os
import re

import pytest

import helpers as H

HDR = os.path.join(H.ROOT, "include", "wf3d.h")


def declared_symbols():
    txt = open(HDR).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(wf3d_[a-z0-9_]+)\s*\(", txt)))


def test_header_symbols_all_exported_and_bound():
    from wf3d import _lib
    lib = _lib.load()
    names = declared_symbols()
    assert len(names) >= 10
    for n in names:
        assert hasattr(lib, n), f"libwf3d.so does not export {n}"
        assert n in _lib.SIGNATURES, f"wf3d/_lib.py has no ctypes signature for {n}"
    assert set(_lib.SIGNATURES) == set(names)
    assert lib.wf3d_version() == 105


def test_library_exports_nothing_but_the_header():
    """exported is a subset of declared too: internal cross-file helpers (the LDS-DMA GEMM back end, the MFMA attention
    kernels, the error formatter) have hidden visibility."""
    import subprocess
    from wf3d import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if "wf3d" in ln.lower()}
    assert exported == set(declared_symbols()), sorted(exported ^ set(declared_symbols()))


def test_library_reads_no_environment():
    """kernel choice is never left to a variable no caller sees: libwf3d.so does not import getenv."""
    import subprocess
    from wf3d import _lib
    out = subprocess.run(["nm", "-D", "--undefined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert not {ln.split()[-1].split("@")[0] for ln in out.splitlines() if ln.strip()} & {"getenv", "secure_getenv"}


def test_set_option_validates():
    from wf3d import _lib
    lib = _lib.load()
    assert lib.wf3d_set_option(b"tn_rounds", 2) == 0
    assert lib.wf3d_set_option(b"tn_rounds", 1) == 0
    assert lib.wf3d_set_option(b"tn_rounds", 9) == -1 and b"1..8" in lib.wf3d_last_error()
    assert lib.wf3d_set_option(b"gemm_cus", 224) == 0 and lib.wf3d_set_option(b"gemm_cus", 0) == 0
    assert lib.wf3d_set_option(b"gemm_cus", 3) == -1 and b"gemm_cus" in lib.wf3d_last_error()
    for v in (3, 6, 1, 0):
        assert lib.wf3d_set_option(b"split_kernel", v) == 0
    for v in (-1, 2, 4, 7):
        assert lib.wf3d_set_option(b"split_kernel", v) == -1 and b"split_kernel" in lib.wf3d_last_error()
    assert lib.wf3d_set_option(b"no_such_switch", 1) == -1 and b"unknown option" in lib.wf3d_last_error()
    assert lib.wf3d_set_option(None, 1) == -1


# Workspace bytes of the split-K GEMM families as recorded before their planners were merged, for every shape bench.py launches
# at cfg1/2/4/5 and shapes on each side of each threshold.  "M,N,K[,layout]:k[/k2]" = k * M * N * 4 bytes (k K ranges; k2 under
# tn_rounds 2 where it differs); "c" = the persistent split kernel's 2048-byte control block.
WS_TABLE = {
    "G": """32,3,256,1:2 32,256,3,0:0 32,256,512,1:4 32,256,4096,0:32 32,512,256,0:2 32,512,512,0:4 32,512,512,1:4
        32,512,1536,1:12 32,1536,512,0:4 128,256,496,2:4 256,3,32,2:0 256,3,512,2:4 256,3,2048,2:16 256,3,8192,2:64
        256,512,496,2:4 496,128,256,0:2 496,256,128,1:0 496,256,512,0:4 496,512,256,1:2 512,3,32,2:0 512,3,256,1:2
        512,3,512,2:4 512,3,2048,2:16 512,3,8192,2:64 512,8,131072,2:128 512,128,4096,0:32 512,256,3,0:0 512,256,32,2:0
        512,256,512,1:4 512,256,512,2:4 512,256,2048,2:16 512,256,8192,2:16 512,512,32,2:0 512,512,256,0:2
        512,512,512,0:4 512,512,512,1:4 512,512,512,2:4 512,512,1536,1:12 512,512,2048,2:8 512,512,8192,2:8
        512,1536,512,0:3 1024,128,224,0:0 1024,128,256,0:2 1024,128,4096,0:32 1536,512,32,2:0 1536,512,512,2:3
        1536,512,2048,2:3 1536,512,8192,2:11 2048,3,256,1:2 2048,128,4096,0:32 2048,256,3,0:0 2048,256,512,1:4
        2048,512,256,0:0 2048,512,512,0:0 2048,512,512,1:0 2048,512,1536,1:0 2048,512,8192,2:8 2048,1536,512,0:0
        8192,3,256,1:2 8192,256,3,0:0 8192,256,512,1:0 8192,512,256,0:0 8192,512,512,0:0 8192,512,512,1:0
        8192,512,1536,1:0 8192,1536,512,0:0 24448,128,4096,0:3 24576,128,4096,0:3 32640,128,4096,0:3 32768,128,4096,0:0""",
    "S": """1000,200,40:c 1000,200,224:c 1000,200,256:2 1024,128,4096:32 1024,512,1024:8 1024,1024,512:4
        1024,1024,2048:16 1024,2048,1024:8 2048,128,4096:32 4096,128,4096:32 4096,512,4104:8 16128,128,256:2
        16128,256,128:c 16128,256,512:4 16128,512,256:c 48896,128,4096:3 49152,128,4096:c 64512,128,256:c
        64512,256,128:c 64512,256,512:c 64512,512,256:c 65280,128,4096:c 65536,128,4096:c 65536,384,512:c
        131072,512,1024:c 131072,1024,512:c 131072,1024,2048:c 131072,2048,1024:c 1044480,128,256:c 1044480,256,128:c
        1044480,256,512:c 1044480,512,256:c""",
    "T": """256,128,16128:56 256,128,64512:224 256,128,1044480:255 256,512,16128:56 256,512,64512:126
        256,512,1044480:128 256,1024,65536:64 256,2048,65536:32 256,4096,65536:16/32 256,48896,65536:2/3
        256,49152,65536:2/3 256,65280,65536:2/3 256,65536,65536:0 512,384,8192:64 512,1024,1024:8 512,1024,131072:32
        1024,128,65536:128 1024,256,224:0 1024,256,256:0 1024,512,1024:8 1024,512,131072:32 1024,2048,1024:8
        1024,2048,131072:8/16 2048,128,65536:64 2048,1024,1024:8 2048,1024,131072:8/16 4096,128,65536:32/64
        48896,128,65536:3/6 49152,128,65536:3/6 65280,128,65536:3/5 65536,128,65536:0""",
}


def test_workspace_sizes_pin_every_split_k_plan():
    from wf3d import _lib
    lib = _lib.load()
    fns = {"G": lib.wf3d_gemm_ws_bytes, "S": lib.wf3d_gemm_split_ws_bytes, "T": lib.wf3d_gemm_split_tn_ws_bytes}
    for r in (1, 2):
        with H.lib_option("tn_rounds", r, default=1):
            for fam, e in ((f, e) for f, entries in WS_TABLE.items() for e in entries.split()):
                a, k = [int(x) for x in e.split(":")[0].split(",")], e.split(":")[1].split("/")[r - 1 if "/" in e else 0]
                assert fns[fam](*a) == (2048 if k == "c" else int(k) * a[0] * a[1] * 4), (fam, e, r)


def test_argument_errors_reported_without_gpu():
    from wf3d import _lib
    lib = _lib.load()
    d = _lib.GemmDesc()
    d.M, d.N, d.K = 4, 4, -1
    assert lib.wf3d_gemm(ctypes.byref(d), None) == -1
    assert b"negative" in lib.wf3d_last_error()
    d.K = 4                                  # null operands
    assert lib.wf3d_gemm(ctypes.byref(d), None) == -1
    assert lib.wf3d_row_stats(None, 4, 0, 0, 1e-5, None, None, None) == -1
    assert lib.wf3d_ln_act_bwd(None, None, 4, 6, None, None, None, None, 0, 0.0, 0, None, None, None, None, None, None, 0, None) == -4
    assert lib.wf3d_gemm_ws_bytes(32, 256, 4096, 0) > 0
    assert lib.wf3d_gemm_ws_bytes(4096, 4096, 64, 0) == 0


def test_struct_layout_matches_header():
    """GemmDesc field order/types must mirror wf3d_gemm_t."""
    from wf3d import _lib
    txt = open(HDR).read()
    body = re.search(r"typedef struct wf3d_gemm_t \{(.*?)\} wf3d_gemm_t;", txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        names = decl.replace("*", " ").split()
        # "int M, N, K" style declarations
        tail = decl.split(None, 1)[1] if not decl.startswith("const") else decl.split(None, 2)[2]
        for nm in tail.split(","):
            fields.append(nm.replace("*", "").strip())
    assert fields == [f[0] for f in _lib.GemmDesc._fields_]


def test_struct_layouts_match_the_compiler(tmp_path):
    """sizeof and every offsetof of the four header structs, as the build's compiler lays them out for the host, against
    the ctypes mirrors derived from the header."""
    import subprocess
    from wf3d import _lib
    assert {c: k.__name__ for c, k in _lib.STRUCTS.items()} == {
        "wf3d_gemm_t": "GemmDesc", "wf3d_skinny_fwd_t": "SkinnyFwd", "wf3d_skinny_bwd_t": "SkinnyBwd", "wf3d_skinny_red_t": "SkinnyRed"}
    assert [len(k._fields_) for k in (_lib.GemmDesc, _lib.SkinnyFwd, _lib.SkinnyBwd, _lib.SkinnyRed)] == [30, 23, 26, 19]
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "wf3d.h"', 'int main() {']
    for c, k in _lib.STRUCTS.items():
        assert issubclass(k, ctypes.Structure)
        lines.append(f'    printf("{c} sizeof %zu\\n", sizeof({c}));')
        lines += [f'    printf("{c} {f[0]} %zu\\n", offsetof({c}, {f[0]}));' for f in k._fields_]
    src, exe = tmp_path / "layout.cpp", tmp_path / "layout"
    src.write_text("\n".join(lines + ["    return 0;", "}", ""]))
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-x", "c++", "-I", os.path.dirname(HDR), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    compiled = {tuple(ln.split()[:2]): int(ln.split()[2]) for ln in out.splitlines()}
    mirrored = {}
    for c, k in _lib.STRUCTS.items():
        mirrored[(c, "sizeof")] = ctypes.sizeof(k)
        mirrored.update({(c, f[0]): getattr(k, f[0]).offset for f in k._fields_})
    assert len(compiled) == 4 + 30 + 23 + 26 + 19
    assert compiled == mirrored, sorted(set(compiled.items()) ^ set(mirrored.items()))


def test_signatures_follow_each_mapping_rule():
    """One entry per rule of the C-type -> ctypes map, written out by hand from include/wf3d.h."""
    from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_long, c_size_t, c_uint32, c_void_p
    from wf3d import _lib
    p, i, f = c_void_p, c_int, c_float
    expect = {
        "wf3d_last_error": (c_char_p, []),
        "wf3d_set_option": (c_int, [c_char_p, c_int]),
        "wf3d_gemm": (c_int, [POINTER(_lib.GemmDesc), c_void_p]),
        "wf3d_gemm_ws_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
        "wf3d_ln_prep": (c_int, [p, i, i, p, p, i, f, f, c_uint32, p, p, p, p]),
        "wf3d_packed_layout_dims": (c_int, [c_int, c_int, POINTER(c_int), POINTER(c_int)]),
        "wf3d_parse_table": (c_long, [c_char_p, c_void_p, c_long, POINTER(c_long)]),
        "wf3d_clip_adam_step": (c_int, [p, p, p, p, p, i, c_double, c_double, c_double, c_double, c_double, c_double, i,
                                        p, c_size_t, p, p]),
        "wf3d_split_rows_multi": (c_int, [p, p, p, p, p, p, i, p]),
    }
    for name, sig in expect.items():
        assert _lib.SIGNATURES[name] == sig, name
    fn = _lib.load().wf3d_clip_adam_step
    assert (fn.restype, list(fn.argtypes)) == expect["wf3d_clip_adam_step"]


MINI_HDR = '#define WF3D_VERSION 105\n#ifdef __cplusplus\nextern "C" {\n#endif\n%s\n#ifdef __cplusplus\n}\n#endif\n'


@pytest.mark.parametrize("decl, names", [
    ("int wf3d_f(const float* x, wchar_t* label, void* stream);", ["wf3d_f", "label", "wchar_t*"]),       # unknown type
    ("int wf3d_f(int n);\nint wf3d_counter;", ["int wf3d_counter"]),                                      # trailing statement
    ("int wf3d_f(int n);\n}", ["}"]),                                                                     # stray text
    ("int wf3d_f(const float*, int n);", ["wf3d_f", "const float*"]),                                     # nameless parameter
    ("int wf3d_f(void (*done)(int), void* stream);", ["wf3d_f", "(*done)"]),                              # function pointer
    ("typedef struct wf3d_gemm_t { const float* A; short M; } wf3d_gemm_t;", ["wf3d_gemm_t.M", "short"]),  # unknown field type
])
def test_parser_refuses_what_it_cannot_map(decl, names):
    from wf3d import _lib
    assert _lib.parse_header(MINI_HDR % "int wf3d_f(const float* x, int n);")[2] == {
        "wf3d_f": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int])}
    with pytest.raises(RuntimeError) as e:
        _lib.parse_header(MINI_HDR % decl)
    for n in names:
        assert n in str(e.value), (n, str(e.value))


def test_load_refuses_a_version_mismatch(monkeypatch):
    """The library must report the WF3D_VERSION of the header the binding came from: the same library under a header text
    that declares the next version is refused as stale."""
    from wf3d import _lib
    txt = open(HDR).read()
    assert "#define WF3D_VERSION 105 " in txt
    defines = _lib.parse_header(txt.replace("#define WF3D_VERSION 105 ", "#define WF3D_VERSION 106 "))[0]
    assert defines["WF3D_VERSION"] == 106 and _lib.DEFINES["WF3D_VERSION"] == 105
    monkeypatch.setattr(_lib, "DEFINES", defines)
    monkeypatch.setattr(_lib, "_lib", None)
    with pytest.raises(RuntimeError, match="stale; rebuild it"):
        _lib.load()
    monkeypatch.undo()
    assert _lib.load().wf3d_version() == _lib.DEFINES["WF3D_VERSION"] == 105


def test_constants_come_from_the_header():
    from wf3d import _lib, ops, skinny
    assert (ops.ACT_NONE, ops.ACT_RELU, ops.ACT_GELU, ops.NT, ops.NN, ops.TN, skinny.MAX_ROWS) == (0, 1, 2, 0, 1, 2, 32)
    assert _lib.DEFINES["WF3D_ERR_UNSUPPORTED"] == -4 and _lib.DEFINES["WF3D_SKINNY_MAX_PROBLEMS"] == 4


def test_ops_reject_cpu_tensors():
    import torch
    from wf3d import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.row_stats(torch.zeros(4, 8))
