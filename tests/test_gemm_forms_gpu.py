"""Every route of wf3d_gemm (csrc/gemm.hip) against fp64, element by element.

The cases, the route each is there for, their data and their fp64 reference are tests/gemm_cases.py (held to the library's
host-side decisions by tests/test_gemm_cases.py).  Each case runs

  * on exact data (small integers; on the bf16x3 routes also the two 16-bit sets on which a missing, doubled or mis-paired
    plane product changes the result): torch.equal against the fp64 result rounded to fp32;
  * on general data (Gaussian, and rows on a large common offset) under a bound per element that is derived, not measured:
        fp32   |got - ref| <= (K + 16) 2^-24 S_ij               K products summed in any order + the epilogue's additions
        x3     |got - ref| <= (3 2^-16 + (K + 16) 2^-24) S_ij   hi + lo leaves <= 2^-16 of each operand; lo.lo is dropped
    with S_ij = sum_k |h_ik||b_kj| + |bias_j| + sum |u||v| + |addend_ij| + |C0_ij| in fp64, plus, under a GELU prologue only,
    the project's element-wise tolerance of the materialising ln_act_apply: 2e-5 max|h| sum_k |b_kj|;

and on both: the poisoned gap columns N..ldc-1 and rows past M keep their bits, a repeated launch gives the same bits, and a
split-K case submitted without a workspace (ws = NULL, or one byte short) runs as one K range — bit-equal on exact data,
inside the bound on general data.  Outputs start as NaN poison, so a tile the XCD remap never visits shows.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import helpers as H  # noqa: E402,F401  (sets sys.path)
import gemm_cases as G  # noqa: E402
import gemm_gpu_util as U  # noqa: E402

POISON, dev, _poisoned, _place, _place1, workspace = U.POISON, U.dev, U.poisoned, U.place, U.place1, U.workspace
NAMES = [c.name for c in G.CASES]


@pytest.fixture(scope="module")
def ops():
    from wf3d import ops as o
    o._lib.load()
    return o


class Staged:
    """A case's operands on the device, at the case's strides and base offsets."""

    def __init__(self, case, inp):
        c = self.case = case
        self.A = _place(inp["A"], c.a_pad, c.a_off)
        self.B = _place(inp["B"], c.b_pad, c.b_off)
        self.bias = _place1(inp["bias"]) if "bias" in inp else None
        self.addend = _place(inp["addend"], c.addend) if "addend" in inp else None
        self.C0 = torch.from_numpy(inp["C0"]).to(dev()) if "C0" in inp else None
        self.lowrank = (_place(inp["U"], c.lr_pad), _place(inp["V"], c.lr_pad)) if "U" in inp else None
        self.pro = None
        if c.pro is not None:
            t = {k: (_place1(inp[k], c.p_off if k in ("gamma", "beta") else 0) if k in inp else None)
                 for k in ("mu", "rs", "gamma", "beta")}
            p, seed = inp.get("drop", (0.0, 0))
            self.pro = (c.pro.act, t["mu"], t["rs"], t["gamma"], t["beta"], p, seed)


def run(ops, st, ws=None, accumulate=None):
    """One launch into a fresh poisoned buffer of M + 2 rows of ldc floats.  Returns (C [M,N] copy, True if every word
    outside C kept its poison)."""
    c = st.case
    acc = c.accumulate if accumulate is None else accumulate
    ldc = c.N + c.ldc_pad
    buf = _poisoned((c.M + 2) * ldc)
    out = buf.view(c.M + 2, ldc)[:c.M, :c.N]
    if acc:
        out.copy_(st.C0)
    with workspace(ops, ws):
        ops.gemm(st.A, st.B, c.layout, bias=st.bias, addend=st.addend, out=out, accumulate=acc,
                 pro=ops.Pro(*st.pro) if st.pro is not None else None, x3=c.x3, lowrank=st.lowrank)
    got = out.clone()
    bits = buf.view(torch.int32).view(c.M + 2, ldc).clone()
    bits[:c.M, :c.N] = POISON
    return got, bool((bits == POISON).all())


def where(case, r, i, j):
    return (f"element ({i}, {j}) = tile ({i // r.bm}, {j // r.bn}) + ({i % r.bm}, {j % r.bn}) of {r.nbm} x {r.nbn} {r.kind} tiles; "
            f"{r.ksplit} K range(s) of {r.kt_per} slices (K = {case.K}, {r.combine} combine), R = {r.R}, body FAST: {r.body}, "
            f"{'x3' if r.x3 else 'fp32'}")


def assert_equal(case, r, got, want, what):
    U.assert_equal(case.name, (r.bm, r.bn), lambda i, j: where(case, r, i, j), got, want, what)


def assert_bound(case, r, got, ref, S, extra, what):
    U.assert_bound(case.name, lambda i, j: where(case, r, i, j), got, ref, G.unit_roundoff_bound(case) * S + extra, S, what)


@pytest.mark.parametrize("name", NAMES)
def test_exact_data_bit_for_bit(ops, name):
    case = G.BY_NAME[name]
    r = case.route()
    for ds in case.exact_sets():
        inp = G.inputs(case, ds)
        ref, _, _ = G.reference(case, inp, True)
        want = torch.from_numpy(ref.astype(np.float32)).to(dev())
        st = Staged(case, inp)
        got, clean = run(ops, st)
        assert_equal(case, r, got, want, ds)
        assert clean, f"{name} [{ds}]: a word outside C[:M, :N] was written (ldc = {case.N + case.ldc_pad})"
        again, _ = run(ops, st)
        assert_equal(case, r, again, got, ds + ", repeated")
        if case.accumulate:
            plain, clean = run(ops, st, accumulate=False)
            assert_equal(case, r, got, plain + st.C0, ds + ", accumulate = plain + C0")
            assert clean
        if r.ksplit > 1:
            for mode in ("null", "short"):
                one, clean = run(ops, st, ws=mode)
                assert_equal(case, case.route(ws_fits=False), one, got, f"{ds}, ws {mode}: one K range")
                assert clean


@pytest.mark.parametrize("data", G.DATA_GENERAL)
@pytest.mark.parametrize("name", NAMES)
def test_general_data_within_the_derived_bound(ops, name, data):
    case = G.BY_NAME[name]
    r = case.route()
    inp = G.inputs(case, data)
    ref, S, extra = G.reference(case, inp, False)
    st = Staged(case, inp)
    got, clean = run(ops, st)
    assert_bound(case, r, got, ref, S, extra, data)
    assert clean, f"{name} [{data}]: a word outside C[:M, :N] was written (ldc = {case.N + case.ldc_pad})"
    again, _ = run(ops, st)
    assert_equal(case, r, again, got, data + ", repeated")
    if r.ksplit > 1:
        one, clean = run(ops, st, ws="null")
        assert_bound(case, case.route(ws_fits=False), one, ref, S, extra, data + ", ws null: one K range")
        short, _ = run(ops, st, ws="short")
        assert_equal(case, case.route(ws_fits=False), short, one, data + ", ws one byte short")
        assert clean


def test_the_workspace_the_wrapper_passes_is_what_the_library_asks_for(ops):
    """The ws modes above lean on ops.gemm sizing its workspace by wf3d_gemm_ws_bytes: a short one must change the route."""
    case = G.BY_NAME["split_ks17_plain"]
    seen = []
    real = ops.scratch

    def spy(nbytes, device, slot=0):
        seen.append(nbytes)
        return real(nbytes, device, slot)
    ops.scratch = spy
    try:
        run(ops, Staged(case, G.inputs(case, "int")))
    finally:
        ops.scratch = real
    assert seen == [G.ws_bytes(case.layout, case.M, case.N, case.K)] and seen[0] > 0
