"""Every kernel form of the split GEMM family (csrc/gemm_split.hip, wf3d_gemm_split_regs in csrc/gemm.hip) against fp64,
element by element, with products = 3 (bf16x3) and products = 1 (bf16 mode).

The cases, the route each is there for, their data and their fp64 reference are tests/split_cases.py (held to the library's
host-side decisions by tests/test_split_cases.py).  The operands are split to sx8 on the host (tests/sx8_model.py), and the
reference is the sum of the plane products each mode defines, so neither split_rows nor the splitting error enters.  Each
case runs

  * on exact data (small integers; with products = 3 also the two 16-bit sets on which a missing, doubled or mis-paired
    plane product changes the result): torch.equal against the fp64 result rounded to fp32;
  * on general data (Gaussian, and rows on a large common offset): |got - ref| <= (K + 16) 2^-24 S_ij per element, S_ij the
    same sum over absolute values (DESIGN.md "wf3d_gemm_split: routes");

and on both: the route query names the kernel form the case is there for, at the very pointers of the launch; the output is a
poisoned buffer of M + 2 rows of ldc floats in which every word outside C[:M, :N] keeps its bits and none inside does; the
operands sit in NaN-poisoned buffers (row padding, and the space behind the last row) and no NaN reaches C; a repeated launch
gives the same bits; a persistent-kernel case gives the bits of the plain 256x256 kernel (with a bias on general data: each
inside the bound, see other_workspaces); and a split-K case submitted
without a workspace (NULL, or one byte short) runs as one K range: bit-equal on exact data, inside the bound on general data.
"""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import helpers as H  # noqa: E402
import gemm_gpu_util as U  # noqa: E402
import split_cases as S  # noqa: E402

NAMES = [c.name for c in S.CASES]


@pytest.fixture(scope="module")
def ops():
    from wf3d import ops as o
    o._lib.load()
    return o


def matmul64(a, b):
    """float64 product on the device (the references of the larger cases would take seconds each on the host)."""
    return (torch.from_numpy(np.ascontiguousarray(a)).to(U.dev()) @ torch.from_numpy(np.ascontiguousarray(b)).to(U.dev())).cpu().numpy()


class Staged:
    """A case's sx8 operands, bias and C0 on the device at the case's strides and base offsets, inside poison."""

    def __init__(self, case, inp):
        self.case = case
        a, b = S.packed(inp)
        self.A = U.place(a, case.a_pad, 0, U.POISON_SX8, tail=64)
        self.B = U.place(b, case.b_pad, 0, U.POISON_SX8, tail=64)
        self.bias = U.place1(inp["bias"], case.bias_off) if case.bias else None
        self.C0 = torch.from_numpy(inp["C0"]).to(U.dev()) if case.accumulate else None


@contextlib.contextmanager
def options(case):
    with H.lib_option("split_kernel", case.split_kernel), H.lib_option("gemm_cus", case.gemm_cus), \
            H.lib_option("tn_rounds", case.tn_rounds, default=1):
        yield


def queried(ops, case, out, bias, ws):
    """The route the library reports for the launch just made (same pointers, same workspace, the device's CU count)."""
    lib = ops._lib.load()
    r = (ctypes.c_int * 8)()
    if case.tn:
        rc = lib.wf3d_gemm_split_tn_route(case.M, case.N, case.K, case.lda, case.ldb, case.ldc, int(case.accumulate), ws[0] or None, ws[1], r)
    else:
        rc = lib.wf3d_gemm_split_route(case.M, case.N, case.K, case.lda, case.ldb, case.ldc, out.data_ptr(),
                                       bias.data_ptr() if bias is not None else None, int(case.accumulate), ws[0] or None, ws[1], 0, r)
    assert rc == 0, lib.wf3d_last_error()
    return list(r)


def run(ops, st, products, ws="case"):
    """One launch into a fresh poisoned buffer of M + 2 rows of ldc floats at the case's base offset.  Returns (C [M, N]
    copy, the model's route of this launch).  Asserts on the way: the library's route query agrees with the model and every
    word outside C kept its poison."""
    c = st.case
    mode = c.ws if ws == "case" else ws
    buf = U.poisoned(c.c_off + (c.M + 2) * c.ldc + 4)
    out = buf[c.c_off:c.c_off + (c.M + 2) * c.ldc].view(c.M + 2, c.ldc)[:c.M, :c.N]
    if c.accumulate:
        out.copy_(st.C0)
    seen = []
    cus = torch.cuda.get_device_properties(U.dev()).multi_processor_count
    with options(c), U.workspace(ops, mode, seen):
        fn = ops.gemm_split_tn if c.tn else ops.gemm_split
        kw = {} if c.tn else dict(bias=st.bias)
        assert (st.A.stride(0), st.B.stride(0), out.stride(0)) == (c.lda, c.ldb, c.ldc)
        fn(st.A, st.B, out=out, accumulate=c.accumulate, products=products, **kw)
        assert len(seen) == 1
        r = c.route_at(*seen[0], out.data_ptr(), st.bias.data_ptr() if st.bias is not None else None, cus)
        got_route = queried(ops, c, out, st.bias, seen[0])
    assert got_route == r.as_query(), f"{c.name}: the library routes {got_route}, the model {r.as_query()} ({r})"
    got = out.clone()
    bits = buf.view(torch.int32).clone()
    inner = bits[c.c_off:c.c_off + (c.M + 2) * c.ldc].view(c.M + 2, c.ldc)
    inner[:c.M, :c.N] = U.POISON
    assert bool((bits == U.POISON).all()), \
        f"{c.name}: a word outside C[:M, :N] was written ({where(c, r, *_first_bad(inner))}; ldc = {c.ldc}, C offset {c.c_off})"
    return got, r


def _first_bad(inner):
    idx = (inner != U.POISON).nonzero()
    return (int(idx[0][0]), int(idx[0][1])) if idx.numel() else (0, 0)


def where(case, r, i, j):
    return (f"element ({i}, {j}) = tile ({i // r.bm}, {j // r.bn}) + ({i % r.bm}, {j % r.bn}) of {r.nbm} x {r.nbn} {r.form} tiles; "
            f"{r.ksplit} K range(s) of {r.kt_per} slices, the last of {r.nks[-1]} (K = {case.K}, {r.combine} combine"
            f"{', zmap' if r.zmap else ''}){f', {r.cus} persistent workgroups' if r.cus else ''}")


def assert_equal(case, r, got, want, what):
    U.assert_equal(case.name, (r.bm, r.bn), lambda i, j: where(case, r, i, j), got, want, what)


def assert_bound(case, r, got, ref, Sabs, what):
    assert not bool(got.isnan().any()), f"{case.name} [{what}]: NaN in C (operand poison read, or output poison left)"
    U.assert_bound(case.name, lambda i, j: where(case, r, i, j), got, ref, S.bound(case) * Sabs, Sabs, what)


def other_workspaces(ops, st, products, r, got, check, exact):
    """The launches that must agree with `got`: a repeat; the plain kernel for a persistent case; one K range for a split.
    The persistent kernel and the plain 256x256 one run the same MFMAs in the same order, so they agree bit for bit — unless
    there is a bias, which the persistent kernel starts its accumulators from and the plain one adds last: then the two
    differ in rounding on general data, and each is held to the bound."""
    c = st.case
    again, _ = run(ops, st, products)
    assert_equal(c, r, again, got, "repeated")
    same_bits = lambda ra, rb: exact or not c.bias or (ra.form == S.X16P) == (rb.form == S.X16P)       # noqa: E731
    if r.form == S.X16P:
        plain, rp = run(ops, st, products, ws="null")
        assert rp.form == S.X16 and rp.ksplit == 1
        if same_bits(r, rp):
            assert_equal(c, rp, plain, got, "plain 256x256 kernel against the persistent one")
        else:
            check(rp, plain, "plain 256x256 kernel")
    if r.ksplit > 1:
        one, r1 = run(ops, st, products, ws="null")
        assert r1.ksplit == 1 and r1.form in (c.form, S.X16)
        check(r1, one, "ws null: one K range")
        short, rs = run(ops, st, products, ws="short")
        assert rs.ksplit == 1
        if same_bits(r1, rs):
            assert_equal(c, rs, short, one, "ws one byte short against ws null")
        else:
            check(rs, short, "ws one byte short: one K range")


@pytest.mark.parametrize("products", S.PRODUCTS)
@pytest.mark.parametrize("name", NAMES)
def test_exact_data_bit_for_bit(ops, name, products):
    case = S.BY_NAME[name]
    for ds in S.exact_sets(products):
        inp = S.inputs(case, ds)
        ref, _ = S.reference(case, inp, products, matmul=matmul64)
        want = torch.from_numpy(ref.astype(np.float32)).to(U.dev())
        st = Staged(case, inp)
        got, r = run(ops, st, products)
        assert r.form == case.form, (name, r)
        assert_equal(case, r, got, want, f"{ds}, products {products}")
        other_workspaces(ops, st, products, r, got, lambda r1, one, what: assert_equal(case, r1, one, got, f"{ds}, {what}"), True)


@pytest.mark.parametrize("products", S.PRODUCTS)
@pytest.mark.parametrize("data", S.G.DATA_GENERAL)
@pytest.mark.parametrize("name", NAMES)
def test_general_data_within_the_derived_bound(ops, name, data, products):
    case = S.BY_NAME[name]
    inp = S.inputs(case, data)
    ref, Sabs = S.reference(case, inp, products, matmul=matmul64)
    st = Staged(case, inp)
    got, r = run(ops, st, products)
    assert r.form == case.form, (name, r)
    assert_bound(case, r, got, ref, Sabs, f"{data}, products {products}")
    other_workspaces(ops, st, products, r, got, lambda r1, one, what: assert_bound(case, r1, one, ref, Sabs, f"{data}, {what}"), False)
