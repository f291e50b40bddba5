"""The route model and the case table of tests/split_cases.py, checked without a GPU:

  * the model against the library: wf3d_gemm_split_ws_bytes, wf3d_gemm_split_tn_ws_bytes, wf3d_gemm_split_tn_ok, and the route
    query wf3d_gemm_split_route / wf3d_gemm_split_tn_route (the function the launch path decides with) for every case, every
    workspace mode, several compute-unit counts, and shapes on both sides of every threshold under every option value;
  * every case reaches the route its `why` names, and every form, combine kind, zmap state and persistent_ok clause has one:
    a retuned threshold fails here instead of silently un-testing a kernel;
  * the exact data sets are exact on the planes the kernels multiply, and the two 16-bit sets tell a dropped, doubled or
    mis-paired plane product from the right arithmetic in every output tile of every case.
"""
import ctypes
import itertools

import numpy as np
import pytest

import helpers as H
import gemm_cases as G
import split_cases as S
from split_cases import DMA3, DMA3_TN, REGS, X16, X16P, X16_TN

ROUTES = [(c, c.route()) for c in S.CASES]
WS_MODES = (None, "null", "short", S.CTL_BYTES, S.CTL_BYTES - 1)
CUS = (256, 304, 8, 64)


@pytest.fixture(scope="module")
def lib():
    from wf3d import _lib
    return _lib.load()


@pytest.fixture
def options():
    """set(opts): the library under the model's options, back to the defaults afterwards."""
    from wf3d import _lib
    lib = _lib.load()

    def set_(o):
        for name, v in (("split_kernel", o.split_kernel), ("gemm_cus", o.gemm_cus), ("tn_rounds", o.tn_rounds)):
            _lib.check(lib.wf3d_set_option(name.encode(), v), name)
    yield set_
    set_(S.Opts())


def query_nt(lib, M, N, K, lda, ldb, ldc, c_addr, bias_addr, accumulate, ws_addr, ws_bytes, cus):
    out = (ctypes.c_int * 8)(*([-1] * 8))
    rc = lib.wf3d_gemm_split_route(M, N, K, lda, ldb, ldc, c_addr, bias_addr, int(accumulate), ws_addr or None, ws_bytes, cus, out)
    assert rc == 0, lib.wf3d_last_error()
    return list(out)


def query_tn(lib, Mo, No, K, lda, ldb, ldc, accumulate, ws_addr, ws_bytes):
    out = (ctypes.c_int * 8)(*([-1] * 8))
    rc = lib.wf3d_gemm_split_tn_route(Mo, No, K, lda, ldb, ldc, int(accumulate), ws_addr or None, ws_bytes, out)
    assert rc == 0, lib.wf3d_last_error()
    return list(out)


def query_case(lib, c, ws_addr, ws_bytes, cus):
    if c.tn:
        return query_tn(lib, c.M, c.N, c.K, c.lda, c.ldb, c.ldc, c.accumulate, ws_addr, ws_bytes)
    return query_nt(lib, c.M, c.N, c.K, c.lda, c.ldb, c.ldc, 0x10000 + 4 * c.c_off, (0x20000 + 4 * c.bias_off) if c.bias else None,
                    c.accumulate, ws_addr, ws_bytes, cus)


# ---- the model against the library -------------------------------------------------------------------------------------
def test_form_and_combine_codes_are_the_headers():
    from wf3d import _lib
    assert [_lib.DEFINES["WF3D_SPLIT_FORM_" + f.upper()] for f in S.FORMS] == list(range(6))
    assert [_lib.DEFINES["WF3D_SPLIT_COMBINE_" + k.upper()] for k in S.COMBINES] == [0, 1, 2]


def test_planner_is_the_general_gemms():
    for tiles, ktotal in itertools.product(range(1, 300, 7), (1, 7, 8, 9, 31, 32, 64, 68, 257, 4096)):
        assert S.splitk_plan(S.RULE_GEMM, tiles, ktotal) == G.splitk_plan(tiles, ktotal)


def test_model_matches_the_library_for_every_case(lib, options):
    for c in S.CASES:
        options(c.opts)
        fn = lib.wf3d_gemm_split_tn_ws_bytes if c.tn else lib.wf3d_gemm_split_ws_bytes
        assert fn(c.M, c.N, c.K) == c.ws_query(), c.name
        if c.tn:
            assert lib.wf3d_gemm_split_tn_ok(c.M, c.N, c.K, c.lda, c.ldb) == 1 and S.tn_ok(c.M, c.N, c.K, c.lda, c.ldb), c.name
        for mode, cus in itertools.product(WS_MODES, CUS):
            for addr, nbytes in {c.ws_given(mode), (c.ws_given(mode)[0] and 8, c.ws_given(mode)[1])}:      # 8: no 16-B / 64-B alignment
                got = query_case(lib, c, addr, nbytes, cus)
                c_addr, b_addr = 0x10000 + 4 * c.c_off, 0x20000 + 4 * c.bias_off
                assert got == c.route_at(addr, nbytes, c_addr, b_addr, cus).as_query(), (c.name, mode, cus, addr, got)


def _shapes_nt():
    out = set()
    for M, N in ((256, 128), (255, 129), (1024, 1024), (768, 1280), (4096, 3072), (4096, 3071), (3840, 3072), (49152, 256), (48896, 256),
                 (49152, 128), (100, 60), (2048, 512), (1000, 200), (1000, 1024), (6144, 2048), (6144, 2047), (65536, 1024)):
        out.update((M, N, K) for K in (8, 32, 104, 192, 224, 232, 256, 264, 288, 320, 2176, 2280, 8192, 16384 + 32))
    return sorted(out)


BASE = dict(ws=(64, S.CTL_BYTES), cus=256, acc=False, c=0x1000, b=0x2000, pads=(0, 0, 0))
# one argument off the base at a time (each persistent_ok clause that an argument can falsify), then a few mixtures
VARIANTS = [{}] + [{k: v} for k, vs in (("ws", ((64, 1 << 40), (32, S.CTL_BYTES), (8, 1 << 40), (0, 0), (0, S.CTL_BYTES), (64, S.CTL_BYTES - 1))),
                                        ("cus", (392, 12, 4, 8, 16)), ("acc", (True,)), ("c", (0x1004,)), ("b", (None, 0x2008)),
                                        ("pads", ((8, 16, 2), (8, 8, 4), (1 << 22, 0, 0), (0, 1 << 22, 0), (0, 0, 1 << 22))))
                   for v in vs] + [dict(ws=(0, 0), acc=True), dict(cus=392, ws=(64, 1 << 40)), dict(c=0x1004, pads=(0, 0, 2))]


def test_model_matches_the_library_around_every_threshold(lib, options):
    seen = set()
    for sk, gc in itertools.product((0, 1, 3, 6), (0, 8, 20)):
        opts = S.Opts(sk, gc, 1)
        options(opts)
        for M, N, K in _shapes_nt():
            assert lib.wf3d_gemm_split_ws_bytes(M, N, K) == S.ws_bytes_nt(M, N, K, opts), (sk, M, N, K)
            for v in VARIANTS:
                a = dict(BASE, **v)
                lda, ldb, ldc = K + a["pads"][0], K + a["pads"][1], N + a["pads"][2]
                args = (M, N, K, lda, ldb, ldc, a["c"], a["b"], a["acc"], *a["ws"], a["cus"])
                r = S.route_nt(*args, opts)
                assert query_nt(lib, *args) == r.as_query(), (opts, args)
                seen.add((r.form, r.ksplit > 1, r.failing[0] if len(r.failing) == 1 else None))
    assert {(f, s) for f, s, _ in seen} >= {(REGS, False), (REGS, True), (DMA3, False), (DMA3, True), (X16, False), (X16, True), (X16P, False)}
    # every clause of persistent_ok is the only false one somewhere in the sweep: a clause the library dropped would show
    # ("cus >= 8" cannot be: a positive count below 8 is no multiple of 8 either)
    names = {n for n, _ in S.persistent_clauses(256, 256, 256, 256, 256, 256, 0, None, False, 1, 64, 2048, 8)}
    assert len(names) == 19 and {f for _, _, f in seen if f} == names - {"cus >= 8"}, names - {f for _, _, f in seen}


def test_tn_model_matches_the_library_around_every_threshold(lib, options):
    seen = set()
    shapes = [(Mo, No, K) for Mo, No in ((256, 128), (256, 256), (256, 384), (512, 512), (768, 256), (1280, 256), (1024, 1024),
                                        (2048, 1024), (4096, 1024), (4096, 4096), (4096, 3840), (256, 2048), (256, 1920))
              for K in (32, 224, 256, 512, 2048, 2080, 2176, 4096, 8192, 65536)]
    for sk, rounds in itertools.product((0, 3, 6), (1, 2, 4)):
        opts = S.Opts(sk, 0, rounds)
        options(opts)
        for Mo, No, K in shapes:
            assert lib.wf3d_gemm_split_tn_ws_bytes(Mo, No, K) == S.ws_bytes_tn(Mo, No, K, opts), (opts, Mo, No, K)
            for ws_addr, ws_bytes in ((64, 1 << 40), (8, 1 << 40), (0, 0), (64, S.ws_bytes_tn(Mo, No, K, opts) - 1)):
                r = S.route_tn(Mo, No, K, ws_addr, max(ws_bytes, 0), opts)
                assert query_tn(lib, Mo, No, K, Mo, No + 4, No, False, ws_addr, max(ws_bytes, 0)) == r.as_query(), (opts, Mo, No, K, ws_addr)
                seen.add((r.form, r.combine, r.zmap))
    assert seen >= {(DMA3_TN, "none", False), (DMA3_TN, "narrow", False), (DMA3_TN, "wide", False), (X16_TN, "none", False),
                    (X16_TN, "narrow", False), (X16_TN, "narrow", True), (X16_TN, "wide", True), (X16_TN, "wide", False)}
    for bad in ((255, 128, 64, 256, 128), (256, 64, 64, 256, 64), (256, 128, 48, 256, 128), (256, 128, 0, 256, 128), (256, 128, 64, 258, 128),
                (256, 128, 64, 256, 130)):
        assert lib.wf3d_gemm_split_tn_ok(*bad) == 0 and not S.tn_ok(*bad), bad


def test_route_query_checks_its_arguments(lib):
    out = (ctypes.c_int * 8)()
    assert lib.wf3d_gemm_split_route(256, 128, 36, 40, 40, 128, None, None, 0, None, 0, 256, out) == -4          # K % 8
    assert lib.wf3d_gemm_split_route(256, 128, 64, 56, 64, 128, None, None, 0, None, 0, 256, out) == -1          # lda < K
    assert lib.wf3d_gemm_split_route(256, 128, 64, 64, 64, 128, None, None, 0, None, 0, 256, None) == -1
    assert lib.wf3d_gemm_split_tn_route(256, 100, 64, 256, 100, 100, 0, None, 0, out) == -4
    assert lib.wf3d_gemm_split_tn_route(256, 128, 64, 256, 128, 124, 0, None, 0, out) == -1


# ---- every case reaches its route; every route has a case -------------------------------------------------------------
def test_every_case_reaches_the_route_it_names():
    for cus in (256, 304, 64):
        for c in S.CASES:
            r = c.route(cus=cus)
            assert r.form == c.form, (c.name, r.form, r.failing)
            assert sum(r.nks) == r.ktotal and min(r.nks) >= 1, c.name
            assert r.nbm * r.bm >= c.M > (r.nbm - 1) * r.bm and r.nbn * r.bn >= c.N > (r.nbn - 1) * r.bn, c.name
            for what in ("nks", "combine", "zmap"):
                assert getattr(c, what) is None or getattr(r, what) == getattr(c, what), (c.name, what, getattr(r, what))
            if c.form == X16P:
                assert not r.failing and r.cus == c.gemm_cus, c.name
            if c.fails is not None:
                assert r.failing == c.fails, (c.name, r.failing)


def test_every_split_case_runs_as_one_range_without_its_workspace():
    n = 0
    for c, r in ROUTES:
        if r.ksplit > 1:
            assert c.ws is None, c.name
            for mode in ("null", "short"):
                one = c.route(ws=mode)
                assert (one.ksplit, one.nks, one.combine, one.zmap) == (1, (r.ktotal,), "none", False), (c.name, mode)
                # one range and a workspace that still holds the control block: the persistent kernel may take it
                assert one.form == c.form or (c.form == X16 and mode == "short" and one.form == X16P and not one.failing), c.name
            n += 1
    assert n >= 20


def _need(what, pred):
    assert [c.name for c, r in ROUTES if pred(c, r)], f"no case reaches: {what}"


def test_every_form_combine_and_zmap_state_has_a_case():
    for f in S.FORMS:
        _need(f, lambda c, r: r.form == f)
        if f != X16P:
            _need((f, "split"), lambda c, r: r.form == f and r.ksplit > 1)
            _need((f, "split, uneven last range"), lambda c, r: r.form == f and r.ksplit > 1 and r.nks[-1] < r.nks[0])
            _need((f, "accumulate"), lambda c, r: r.form == f and c.accumulate)
            _need((f, "accumulate through the combine"), lambda c, r: r.form == f and c.accumulate and r.ksplit > 1)
            _need((f, "ldc > N"), lambda c, r: r.form == f and c.ldc_pad)
        _need((f, "padded operand rows"), lambda c, r: r.form == f and c.a_pad and c.b_pad)
    for f in (DMA3, X16, DMA3_TN, X16_TN):
        _need((f, "wide"), lambda c, r: r.form == f and r.combine == "wide")
        _need((f, "narrow"), lambda c, r: r.form == f and r.combine == "narrow")
    _need("regs: more than 16 ranges, N % 4 == 0, narrow", lambda c, r: r.form == REGS and r.ksplit > 16 and c.N % 4 == 0 and r.combine == "narrow")
    _need("more than 16 ranges, N % 4 != 0: narrow", lambda c, r: r.form == DMA3 and r.ksplit > 16 and c.N % 4 and r.combine == "narrow")
    _need("zmap on one tile", lambda c, r: r.zmap and r.nbm * r.nbn == 1)
    _need("zmap on several tiles, 16 ranges", lambda c, r: r.zmap and r.nbm * r.nbn > 1 and r.ksplit == 16)
    _need("zmap, short last range", lambda c, r: r.zmap and r.nks[-1] < r.nks[0])
    _need("x16_tn split without zmap", lambda c, r: r.form == X16_TN and r.ksplit > 1 and not r.zmap)
    _need("tn_rounds changes the plan", lambda c, r: c.tn and c.tn_rounds == 2 and r.nbm * r.nbn >= 16
          and S.route_tn(c.M, c.N, c.K).ksplit != r.ksplit)
    # bias with and without split-K, with accumulate in each
    for f in (DMA3, X16):
        for split, acc in itertools.product((False, True), repeat=2):
            _need((f, "bias", "split" if split else "one range", "accumulate" if acc else "overwrite"),
                  lambda c, r: r.form == f and c.bias and (r.ksplit > 1) == split and c.accumulate == acc)


def test_every_edge_the_kernels_have_has_a_case():
    # pipeline prologue and `ahead` edges: 1, 2, 3 (and 4) slices in one range on every LDS-DMA form
    for f, want in ((DMA3, {1, 2, 3, 4}), (X16, {1, 2, 3}), (DMA3_TN, {1, 2, 3}), (X16_TN, {1, 2, 3})):
        got = {r.nks[0] for c, r in ROUTES if r.form == f and r.ksplit == 1}
        assert got >= want, (f, sorted(got))
    assert {c.K for c, r in ROUTES if r.form == REGS and c.K % 32} >= {8, 40, 104}
    _need("regs on K % 32 == 0", lambda c, r: r.form == REGS and c.K % 32 == 0 and c.split_kernel == 1)
    _need("regs: N % 4 != 0 in a partial tile", lambda c, r: r.form == REGS and c.N % 4 and c.N % 128 and c.M % 128)
    _need("dma3: M % 256", lambda c, r: r.form == DMA3 and c.M % 256)
    _need("dma3: N % 128", lambda c, r: r.form == DMA3 and c.N % 128 and c.N % 4 == 0)
    _need("dma3: N % 4", lambda c, r: r.form == DMA3 and c.N % 4)
    _need("x16: 256 x 256 x 32", lambda c, r: r.form == X16 and (c.M, c.N, c.K) == (256, 256, 32))
    _need("x16: partial tiles both ways", lambda c, r: r.form == X16 and c.M % 256 and c.N % 256)
    _need("x16: misaligned C", lambda c, r: r.form == X16 and c.c_off % 4 and c.ldc % 4 == 0 and c.accumulate)
    _need("x16: ldc % 4", lambda c, r: r.form == X16 and c.ldc % 4 and c.c_off == 0)
    _need("x16: slabs with N % 4 != 0", lambda c, r: r.form == X16 and r.ksplit > 1 and c.N % 4)
    _need("dma3_tn: No % 256", lambda c, r: r.form == DMA3_TN and c.N % 256)
    _need("dma3_tn forced", lambda c, r: r.form == DMA3_TN and c.N % 256 == 0 and c.split_kernel == 3)
    _need("dma3 forced", lambda c, r: r.form == DMA3 and c.N % 256 == 0 and c.split_kernel == 3)
    # a tile count that does not divide over the 8 XCDs, on every form with an XCD remap
    for f in (DMA3, X16, X16P, DMA3_TN):
        _need((f, "tiles % 8"), lambda c, r: r.form == f and (r.nbm * r.nbn) % 8 and r.nbm * r.nbn > 1)
    # the persistent kernel's own edges
    p = [(c, r) for c, r in ROUTES if r.form == X16P]
    assert {c.K for c, _ in p} >= {256, 320} and {c.bias for c, _ in p} == {False, True}
    _need("x16p: exactly 2 x cus tiles", lambda c, r: r.form == X16P and r.nbm * r.nbn == 2 * r.cus)
    _need("x16p: tiles % 8 != 0", lambda c, r: r.form == X16P and (r.nbm * r.nbn) % 8)
    _need("x16p: one tile column", lambda c, r: r.form == X16P and r.nbn == 1)
    _need("x16p: 16 workgroups, >= 32 tiles", lambda c, r: r.form == X16P and r.cus == 16 and r.nbm * r.nbn >= 32)
    _need("x16p: padded rows", lambda c, r: r.form == X16P and c.a_pad and c.b_pad and c.ldc_pad)


def test_every_reachable_persistent_clause_fails_alone_in_a_case():
    """Each fallback case is a persistent case but for its clause: the same call with the clause mended is persistent."""
    alone = {r.failing[0] for c, r in ROUTES if c.fails is not None and len(r.failing) == 1}
    assert alone >= {"one K range", "no accumulate", "M % 256", "N % 256", ">= 8 slices", "even slice count", "control block fits",
                     ">= 2 tiles per workgroup", "ldc % 4", "C % 16", "bias % 16"}, alone
    _need("no workspace at all", lambda c, r: c.fails is not None and "workspace" in r.failing)
    _need("7 slices", lambda c, r: c.fails is not None and r.ktotal == 7)
    for c, r in ROUTES:
        if c.fails is not None:
            assert r.form == X16 and c.split_kernel == 6 and c.gemm_cus == 8, c.name


def test_cases_are_small():
    for c in S.CASES:
        assert c.M * c.N <= 25e6 and c.M * c.N * c.K <= 2.5e9, c.name


# ---- the data ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exact_products():
    """{(case name, data set): (plane products, plane products of the absolute values)} for the exact sets, computed once."""
    out = {}
    for c in S.CASES:
        for ds in G.DATA_EXACT:
            inp = S.inputs(c, ds)
            out[c.name, ds] = (inp, S.plane_products(c, inp), S.plane_products(c, inp, absolute=True))
    return out


def test_exact_data_sets_are_exact(exact_products):
    """Every plane value is an integer and no sum of absolute plane products (plus bias and C0) reaches 2^24: every partial
    sum, in any order, over any subset of the products, is an fp32 number on the grid of the lowest lo-plane bit (1)."""
    for (name, ds), (inp, pp, pa) in exact_products.items():
        c = S.BY_NAME[name]
        for x in S.planes(c, inp):
            assert np.array_equal(x, np.round(x)), (name, ds)
        for products in S.PRODUCTS:
            if ds not in S.exact_sets(products):
                continue
            w = S.X3 if products == 3 else S.X1
            epi = [inp[k].astype(np.float64) if k == "C0" else inp[k].astype(np.float64)[None, :] for k in ("bias", "C0") if k in inp]
            ref, Sabs = sum(w[k] * pp[k] for k in w) + sum(epi), sum(w[k] * pa[k] for k in w) + sum(np.abs(e) for e in epi)
            assert Sabs.max() < 2 ** 24, (name, ds, products, Sabs.max())
            assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref), (name, ds, products)
        # the 16-bit operand has both planes live wherever it is non-zero, the other one no low part
        if ds in ("x3a", "x3b"):
            ph, pl, qh, ql = S.planes(c, inp)
            big, small = ((ph, pl), (qh, ql)) if ds == "x3a" else ((qh, ql), (ph, pl))
            assert np.all(big[0] != 0) and np.all(big[1] != 0) and not small[1].any() and small[0].any(), (name, ds)


MUTANTS = {"al.bh dropped": ({"hh": 1, "hl": 1, "lh": 0, "ll": 0}, ("x3a",)),
           "ah.bl dropped": ({"hh": 1, "hl": 0, "lh": 1, "ll": 0}, ("x3b",)),
           "ah.bh doubled": ({"hh": 2, "hl": 1, "lh": 1, "ll": 0}, ("x3a", "x3b")),
           "al paired with bl": ({"hh": 1, "hl": 1, "lh": 0, "ll": 1}, ("x3a",)),
           "bl paired with al": ({"hh": 1, "hl": 0, "lh": 1, "ll": 1}, ("x3b",))}


def test_the_16_bit_sets_tell_wrong_plane_products_apart(exact_products):
    """On x3a / x3b a dropped cross product, a doubled hi.hi and a lo paired with a lo each change the reference of every
    case, in every output tile of the form the case runs on."""
    for c, r in ROUTES:
        for what, (w, sets) in MUTANTS.items():
            for ds in sets:
                _, pp, _ = exact_products[c.name, ds]
                diff = sum((w[k] - S.X3[k]) * pp[k] for k in w if w[k] != S.X3[k]) != 0
                for ti, tj in itertools.product(range(r.nbm), range(r.nbn)):
                    assert diff[ti * r.bm:(ti + 1) * r.bm, tj * r.bn:(tj + 1) * r.bn].any(), (c.name, ds, what, "tile", ti, tj)


def test_bound_is_the_general_gemms_accumulation_term():
    for c in S.CASES:
        g = S.as_gemm_case(c)
        assert S.bound(c) == G.unit_roundoff_bound(g) == (c.K + 16) * 2.0 ** -24
