"""The resident data set entry points of csrc/cloud.hip without a GPU: the argument checks of wf3d_cloud_normalize,
wf3d_cloud_sample, wf3d_cloud_pack and wf3d_wireframe_targets (every refusal comes before the launch, so host addresses
stand in for device memory and nothing is read through them), and the host parser wf3d_parse_table / wf3d_parse_floats
against np.loadtxt, whose semantics datasets.building3d._read_xyz documents: the same array, or both raise."""
import ctypes
import warnings

import numpy as np
import pytest

import helpers as H  # noqa: F401  (the package path)


@pytest.fixture(scope="module")
def lib():
    from wf3d import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def addr():
    """a 64-byte aligned host address; never read by a call that is refused"""
    store = np.zeros(1024, dtype=np.uint8)
    a = store.ctypes.data
    yield a + -a % 64                                    # `store` lives until the module's tests are done


def _codes():
    from wf3d import _lib
    return _lib.DEFINES["WF3D_OK"], _lib.DEFINES["WF3D_ERR_ARG"], _lib.DEFINES["WF3D_ERR_UNSUPPORTED"]


def _refused(lib, name, message, call, args, cases, code):
    """every case is refused with `code`, and wf3d_last_error() is this entry point's message for this kind of refusal
    (the kinds alternate from call to call, so a message left over from the refusal before cannot pass)"""
    for kw in cases:
        assert call(dict(args, **kw)) == code, (name, kw)
        assert lib.wf3d_last_error() == f"{name}: {message}".encode(), (name, kw, lib.wf3d_last_error())


def test_cloud_normalize_argument_checks(lib, addr):
    OK, ERR_ARG, _ = _codes()
    args = dict(raw=addr, first=addr, nclouds=2, C=8, lo=3, hi=7, normalize=1, out=addr, centroid=addr, md=addr)

    def call(a):
        return lib.wf3d_cloud_normalize(a["raw"], a["first"], a["nclouds"], a["C"], a["lo"], a["hi"], a["normalize"], a["out"],
                                        a["centroid"], a["md"], None)
    for dims, null in zip((dict(C=2), dict(C=17), dict(nclouds=-1), dict(C=0), dict(C=-8)),
                          (dict(raw=None), dict(first=None), dict(out=None), dict(centroid=None), dict(md=None))):
        _refused(lib, "wf3d_cloud_normalize", "bad dims", call, args, (dims,), ERR_ARG)
        _refused(lib, "wf3d_cloud_normalize", "null pointer", call, args, (null,), ERR_ARG)
    # no cloud: nothing to do, nothing read (every pointer NULL)
    assert call(dict(args, nclouds=0, raw=None, first=None, out=None, centroid=None, md=None)) == OK


def test_cloud_sample_argument_checks(lib, addr):
    OK, ERR_ARG, ERR_UNSUPPORTED = _codes()
    args = dict(norm=addr, first=addr, cloud=addr, choice=addr, aug=addr, B=2, P=4, C=8, out=addr)

    def call(a):
        return lib.wf3d_cloud_sample(a["norm"], a["first"], a["cloud"], a["choice"], a["aug"], a["B"], a["P"], a["C"], a["out"], None)
    for dims, null in zip((dict(C=2), dict(C=17), dict(B=-1), dict(P=-1), dict(C=0), dict(B=65536, C=2)),
                          (dict(norm=None), dict(first=None), dict(cloud=None), dict(choice=None), dict(aug=None), dict(out=None))):
        _refused(lib, "wf3d_cloud_sample", "bad dims", call, args, (dims,), ERR_ARG)
        _refused(lib, "wf3d_cloud_sample", "null pointer", call, args, (null,), ERR_ARG)
    _refused(lib, "wf3d_cloud_sample", "B > 65535", call, args, (dict(B=65536),), ERR_UNSUPPORTED)
    nulls = dict(norm=None, first=None, cloud=None, choice=None, aug=None, out=None)
    assert call(dict(args, B=0, **nulls)) == OK and call(dict(args, P=0, **nulls)) == OK          # an empty batch: nothing read


def test_cloud_pack_argument_checks(lib, addr):
    _, ERR_ARG, _ = _codes()
    args = dict(norm=addr, first=addr, nclouds=2, params=addr, B=2, capacity=256, C=8, points=addr, counts=addr)

    def call(a):
        return lib.wf3d_cloud_pack(a["norm"], a["first"], a["nclouds"], a["params"], a["B"], a["capacity"], a["C"], a["points"],
                                   a["counts"], None)
    groups = {"bad dims": (dict(C=2), dict(C=17), dict(B=0), dict(B=4097), dict(capacity=0), dict(nclouds=0)),
              "null pointer": (dict(norm=None), dict(first=None), dict(params=None), dict(points=None), dict(counts=None)),
              "params must be 8-byte aligned": (dict(params=addr + 4), dict(C=3, params=addr + 4), dict(C=7, params=addr + 1)),
              "norm and points must be 16-byte aligned": (dict(norm=addr + 8), dict(points=addr + 8), dict(points=addr + 4))}
    for k in range(6):                                   # one case of each kind in turn
        for message, cases in groups.items():
            if k < len(cases):
                _refused(lib, "wf3d_cloud_pack", message, call, args, (cases[k],), ERR_ARG)


def test_wireframe_targets_argument_checks(lib, addr):
    _, ERR_ARG, _ = _codes()
    args = dict(wfv=addr, wfe=addr, vfirst=addr, efirst=addr, nclouds=2, params=addr, B=2, V=8, vertices=addr, existence=addr,
                counts=addr, labels=addr)

    def call(a):
        return lib.wf3d_wireframe_targets(a["wfv"], a["wfe"], a["vfirst"], a["efirst"], a["nclouds"], a["params"], a["B"], a["V"],
                                          a["vertices"], a["existence"], a["counts"], a["labels"], None)
    groups = {"bad dims": (dict(B=0), dict(B=4097), dict(V=0), dict(V=32769), dict(nclouds=0)),
              "null pointer": (dict(vfirst=None), dict(efirst=None), dict(params=None), dict(vertices=None), dict(existence=None),
                               dict(counts=None), dict(labels=None), dict(labels=None, V=2)),
              "params must be 8-byte aligned": (dict(params=addr + 4), dict(params=addr + 1), dict(V=1, labels=None, params=addr + 2))}
    for k in range(8):                                   # one case of each kind in turn
        for message, cases in groups.items():
            if k < len(cases):
                _refused(lib, "wf3d_wireframe_targets", message, call, args, (cases[k],), ERR_ARG)


# ---------------------------------------------------------------------------------------------------------------------
# the parser
# ---------------------------------------------------------------------------------------------------------------------
ACCEPTED = {
    "no trailing newline": "1 2 3\n4 5 6",
    "CRLF": "1 2 3\r\n4 5 6\r\n",
    "tabs": "1\t2\t3\n4\t5\t6\n",
    "blank lines holding spaces": "1 2 3\n   \n \t \n4 5 6\n\n",
    "comment-only file": "# a\n  # b\n",
    "empty file": "",
    "comment at end of file without newline": "1 2 3\n4 5 6\n# end",
    "comment behind a number": "1 2#c\n3 4 # d\n",
    "+1.5": "+1.5 2 3\n4 5 6\n",
    ".5": ".5 2 3\n4 5 -.5\n",
    "5.": "5. 2 3\n4 5 6.\n",
    "1E5": "1E5 2e-3 3\n4 5 6E+2\n",
    "inf": "inf 2 3\n4 5 6\n",
    "-inf": "-inf 2 3\n4 5 6\n",
    "nan": "nan 2 3\n4 5 6\n",
    "1e400": "1e400 2 3\n4 5 -1e400\n",
    "a lone CR ends a row": "1 2\r3 4\r",
    "a lone CR ends a comment": "1 2 # c\r3 4",
    "CR CR LF": "1 2\r\r\n3 4\n",
    "vertical tab and form feed are whitespace": "1\v2\f3\n4 5 6\n",
    "one value": "7.25",
    "one row": "1 2 3 4 5 6 7 8\n",
    "17 digits": "532215.38000000000 6589285.6500000004 7.6699999999999999\n0.1 0.2 0.30000000000000004\n",
}
REJECTED = {
    "3.4.5": "1 2 3.4.5\n",
    "3.4.5 read as two values": "1 2 3.4.5\n1 2 3 4\n",
    "1.0-2.0": "1.0-2.0 3\n",
    "0x10": "0x10 2 3\n",
    "-0X1p3": "1 -0X1p3 3\n",
    "1e5x": "1e5x 2\n",
    "1,2,3": "1,2,3\n",
    "1d5": "1d5 2\n",
    "nan(1)": "nan(1) 2\n",
    "a word": "1 2 three\n",
    "a bad last token without newline": "1 2 3\n4 5 6.0.0",
}


def _loadtxt(path):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                  # "input contained no data"
        return np.loadtxt(path, dtype=np.float64)


@pytest.mark.parametrize("name", list(ACCEPTED))
def test_parser_accepts_what_loadtxt_accepts(tmp_path, name, lib):
    """`lib`: _read_xyz falls back to np.loadtxt when the library cannot be loaded; here that is an error"""
    from datasets.building3d import _read_xyz
    p = tmp_path / "a.xyz"
    p.write_bytes(ACCEPTED[name].encode())
    want = _loadtxt(str(p))
    got = _read_xyz(str(p))
    assert got.dtype == np.float64 and got.ndim == 2
    if want.size == 0:
        assert got.size == 0 and got.shape[0] == 0
    else:
        want = np.atleast_2d(want)
        assert got.shape == want.shape and np.array_equal(got, want, equal_nan=True), (got, want)
        assert np.array_equal(np.signbit(got), np.signbit(want))


@pytest.mark.parametrize("name", list(REJECTED))
def test_parser_rejects_what_loadtxt_rejects(tmp_path, name, lib):
    from datasets.building3d import _read_xyz
    p = tmp_path / "r.xyz"
    p.write_bytes(REJECTED[name].encode())
    with pytest.raises(ValueError):
        _loadtxt(str(p))
    with pytest.raises(OSError, match=r"cannot parse .* \(code -2\)"):
        _read_xyz(str(p))
    assert lib.wf3d_parse_floats(str(p).encode(), None, 0) == -2


def test_parser_second_call_with_a_larger_buffer(tmp_path, lib):
    """3000 values in 6000 bytes: more than _read_xyz's first buffer (max(1024, bytes / 4) = 1500), so it calls again"""
    from datasets.building3d import _read_xyz
    p = tmp_path / "big.xyz"
    want = (np.arange(3000) % 10).astype(np.float64).reshape(1000, 3)
    p.write_text("".join("%d %d %d\n" % tuple(r) for r in want))
    assert p.stat().st_size == 6000
    got = _read_xyz(str(p))
    assert got.shape == (1000, 3) and np.array_equal(got, want) and np.array_equal(got, _loadtxt(str(p)))
    # the ABI: the count comes back whatever the buffer holds; only out[0 .. max_vals) is written
    path, cols = str(p).encode(), ctypes.c_long(-1)
    assert lib.wf3d_parse_floats(path, None, 0) == 3000
    assert lib.wf3d_parse_floats(path, None, 5000) == 3000
    buf = np.full(16, -7.0)
    assert lib.wf3d_parse_table(path, buf.ctypes.data_as(ctypes.c_void_p), 10, ctypes.byref(cols)) == 3000 and cols.value == 3
    assert np.array_equal(buf[:10], want.reshape(-1)[:10]) and (buf[10:] == -7.0).all()
    assert lib.wf3d_parse_floats(path, buf.ctypes.data_as(ctypes.c_void_p), 0) == 3000 and (buf[10:] == -7.0).all()
    assert lib.wf3d_parse_table(path, None, 0, None) == -1                                        # ncols is required
    assert lib.wf3d_parse_floats(str(tmp_path / "missing.xyz").encode(), None, 0) == -1
