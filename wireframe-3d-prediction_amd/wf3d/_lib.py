"""ctypes binding of libwf3d.so, derived from its C ABI: include/wf3d.h is parsed when this module is imported and
yields DEFINES (the `#define` integers), the struct mirrors and SIGNATURES.  Nothing is declared here by hand.

The HIP library is the product path.  There is NO fallback: if the header or the shared object is missing, a
declaration cannot be mapped or a symbol is absent, importing / loading raises.
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("WF3D_LIB", os.path.join(os.path.dirname(_HERE), "libwf3d.so"))   # override: timing-only ablation builds
HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "wf3d.h")    # what csrc/ compiles against

_SCALARS = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float, "double": ctypes.c_double,
            "size_t": ctypes.c_size_t, "uint32_t": ctypes.c_uint32}
# what a pointer that travels as a plain address (c_void_p: device memory, host tables) may point to
_POINTEES = {"void", "float", "double", "int", "long", "int32_t", "int64_t", "uint32_t", "uint64_t", "unsigned char"}
_STRUCT_CLASSES = {"wf3d_gemm_t": "GemmDesc", "wf3d_skinny_fwd_t": "SkinnyFwd", "wf3d_skinny_bwd_t": "SkinnyBwd",
                   "wf3d_skinny_red_t": "SkinnyRed"}
_TYPE_WORDS = {w for t in (*_SCALARS, *_POINTEES, "char", "const") for w in t.split()}


def _fail(msg):
    raise RuntimeError("wf3d: include/wf3d.h: " + msg)


def _ctype(spelling, structs, where):
    """The ctypes type of one C type spelling: scalars by name; `const char*` -> c_char_p; a pointer to a header struct
    -> POINTER(its class); a non-const `int*` / `long*` (host out-parameter) -> POINTER(c_int / c_long); every other
    pointer to a known type -> c_void_p (device memory and host tables travel as plain addresses)."""
    tok = re.findall(r"\w+|\*", spelling)
    stars = tok.count("*")
    head, tail = (tok[:tok.index("*")], tok[tok.index("*"):]) if stars else (tok, [])
    const, base = "const" in head, " ".join(t for t in head if t != "const")
    if "".join(tok) == spelling.replace(" ", "") and not set(tail) - {"*", "const"}:
        if not stars and not const and base in _SCALARS:
            return _SCALARS[base]
        if tail == ["*"] and base == "char" and const:
            return ctypes.c_char_p
        if tail == ["*"] and base in structs:
            return ctypes.POINTER(structs[base])
        if tail == ["*"] and base in ("int", "long") and not const:
            return ctypes.POINTER(_SCALARS[base])
        if stars and base in _POINTEES:
            return ctypes.c_void_p
    _fail(f"{where}: no ctypes mapping for the type `{spelling}`")


def _declarator(text, where):
    """`<type> <name>` -> (type spelling, name)."""
    text = " ".join(text.split())
    if "(" in text or ")" in text:
        _fail(f"{where}: function-pointer parameter `{text}` is not supported")
    m = re.fullmatch(r"(.*?)\s*\b([A-Za-z_]\w*)", text)
    if not m or not m.group(1) or m.group(2) in _TYPE_WORDS:
        _fail(f"{where}: parameter `{text}` has no name")
    return m.groups()


def _struct(name, body, structs):
    """The ctypes.Structure of `typedef struct name { body } name;`.  `int M, N, K;` declares three fields, `void* slabs[3]` an array."""
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        first, *more = decl.split(",")
        spelling = _declarator(re.sub(r"\[\d+\]", "", first), name)[0]
        if more and "*" in spelling:
            _fail(f"{name}: `{decl}` declares several pointers in one statement")
        for d in (first, *(f"{spelling} {m}" for m in more)):
            d, dim = re.fullmatch(r"(.*?)(?:\[(\d+)\])?", d.strip(), flags=re.S).groups()
            spelling, field = _declarator(d, name)
            ctype = _ctype(spelling, structs, f"{name}.{field}")
            fields.append((field, ctype * int(dim) if dim else ctype))
    return type(_STRUCT_CLASSES[name], (ctypes.Structure,), {"_fields_": fields, "__doc__": f"Mirror of `{name}` (include/wf3d.h)."})


def parse_header(text):
    """(defines, structs, signatures) of a header text: the `#define NAME <int>` values by name, a ctypes.Structure per
    `typedef struct` block by C name, and name -> (restype, [argtypes]) of every prototype.  Strict: with the comments,
    the preprocessor lines, the extern "C" wrapper and the typedef blocks taken out, every remaining statement must be
    a prototype whose types all map; anything else raises and names the text."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    defines = {}
    for line in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(.*)$", text, flags=re.M):
        m = re.fullmatch(r"(\w+)(?:\s+\(?(-?\d+)\)?)?\s*", line) or _fail(f"cannot parse `#define {line.strip()}`")
        if m.group(2) is not None:
            defines[m.group(1)] = int(m.group(2))
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    m = re.fullmatch(r'(.*?)extern\s+"C"\s*\{(.*)\}\s*', text, flags=re.S) or _fail('no extern "C" { ... } around the declarations')
    structs = {}

    def typedef(m):
        if m.group(1) != m.group(3) or m.group(1) not in _STRUCT_CLASSES:
            _fail(f"struct `{m.group(1)}` / `{m.group(3)}` has no class name in wf3d/_lib.py")
        structs[m.group(1)] = _struct(m.group(1), m.group(2), structs)
        return ""
    text = re.sub(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", typedef, m.group(1) + m.group(2), flags=re.S)
    signatures = {}
    for stmt in filter(None, (" ".join(s.split()) for s in text.split(";"))):
        m = re.fullmatch(r"(.+?)\b([A-Za-z_]\w*) ?\((.*)\)", stmt) or _fail(f"cannot parse `{stmt}` as a function prototype")
        ret, name, params = (g.strip() for g in m.groups())
        params = [] if params == "void" else [_declarator(p, f"{name}, parameter {i + 1}") for i, p in enumerate(params.split(","))]
        signatures[name] = (_ctype(ret, structs, f"{name}, return type"),
                            [_ctype(spelling, structs, f"{name}, parameter `{pname}`") for spelling, pname in params])
    return defines, structs, signatures


try:
    with open(HEADER_PATH) as _f:
        DEFINES, STRUCTS, SIGNATURES = parse_header(_f.read())
except OSError as _e:
    raise RuntimeError(f"wf3d: {HEADER_PATH} not found — the binding of libwf3d.so is derived from the header it was "
                       "compiled against (include/wf3d.h of the source tree)") from _e
GemmDesc, SkinnyFwd, SkinnyBwd, SkinnyRed = (STRUCTS[n] for n in _STRUCT_CLASSES)

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
    # same names with older argument lists are what a derived binding cannot see: the library must be the header's
    if lib.wf3d_version() != DEFINES["WF3D_VERSION"]:
        raise RuntimeError(f"wf3d: libwf3d.so is stale; rebuild it (it reports version {lib.wf3d_version()}, "
                           f"include/wf3d.h declares {DEFINES['WF3D_VERSION']})")
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
