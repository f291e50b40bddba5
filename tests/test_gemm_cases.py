"""The route model and the case table of tests/gemm_cases.py, checked without a GPU:

  * the model's split-K plan and tile kind against the library's own wf3d_gemm_ws_bytes (host-only), for every case and
    for shapes on both sides of every threshold;
  * every route that tests/test_gemm_forms_gpu.py is there for has a case: a retuned threshold fails here instead of
    silently un-testing a route;
  * the exact data sets are exact: every partial sum representable, the prologue exact in fp32, the fp64 reference its own
    fp32 rounding, and on the x3 sets hi + lo = value with the cross products the kernel keeps summing to the product.
"""
import dataclasses
import itertools

import numpy as np
import pytest

import helpers as H  # noqa: F401  (sets sys.path)
import gemm_cases as G
import sx8_model
from gemm_cases import BIG, MID, NN, NT, SMALL, TN

ROUTES = [(c, c.route()) for c in G.CASES]


@pytest.fixture(scope="module")
def lib():
    from wf3d import _lib
    return _lib.load()


# ---- the model against the library -------------------------------------------------------------------------------------
def test_layout_and_activation_codes_are_the_headers():
    from wf3d import _lib
    assert (G.NT, G.NN, G.TN) == tuple(_lib.DEFINES["WF3D_" + n] for n in ("NT", "NN", "TN"))
    assert (G.ACT_NONE, G.ACT_RELU, G.ACT_GELU) == tuple(_lib.DEFINES["WF3D_ACT_" + n] for n in ("NONE", "RELU", "GELU"))


def test_model_workspace_matches_library_for_every_case(lib):
    for c, r in ROUTES:
        assert lib.wf3d_gemm_ws_bytes(c.M, c.N, c.K, c.layout) == G.ws_bytes(c.layout, c.M, c.N, c.K) \
            == (r.planned * c.M * c.N * 4 if r.planned > 1 else 0), c.name


def _threshold_shapes():
    """Shapes on both sides of each host-side threshold, each with a K that splits (so the tile kind enters the answer)."""
    out = set()
    ks = (224, 255, 256, 257, 288, 2048, 2049, 4096, 4097, 512)          # ktotal = 7 / 8 / 9, K = 2048/2049, 4096/4097
    for M in (1, 31, 32, 33, 63, 64, 65, 127, 128, 129):
        for N in (1, 63, 64, 65, 128, 129, 1000):
            out.update((M, N, K) for K in ks)
    # t64 = 127 / 128 (and t128 well under 256): 127 = 127 x 1, 128 = 8 x 16 = 2 x 64
    for M, N in ((127 * 64, 64), (127 * 64 + 1, 64), (512, 1024), (512, 960), (449, 961), (448, 1024), (128, 4096), (128, 4032),
                 (65, 4096), (65, 4032), (2048, 256), (1984, 256)):
        out.update((M, N, K) for K in ks)
    # t128 = 255 / 256, 63 / 64, 16 / 17
    for M, N in ((255 * 128, 128), (255 * 128 + 1, 128), (2048, 2048), (2048, 2040), (2048, 1920), (1920, 2048 + 128), (1024, 1024),
                 (1024, 1023), (1024, 896), (1008, 1024), (512, 512), (512, 513), (513, 512), (2176, 128), (2177, 128)):
        out.update((M, N, K) for K in (256, 2048, 2049, 4096, 4097, 8192))
    # tiles = 8 / 9 (few_tiles) on each tile kind, ktotal around the 4-slice minimum
    for M, N in ((64, 512), (64, 513), (33, 512), (32, 1025), (1024, 128), (1025, 128), (1024, 64), (384, 384), (385, 384), (192, 192),
                 (129, 192), (193, 192)):
        out.update((M, N, K) for K in (255, 256, 257, 1024, 2176, 2177, 8192, 8193, 16384, 40000))
    return sorted(out)


def test_model_workspace_matches_library_around_every_threshold(lib):
    shapes = _threshold_shapes()
    assert len(shapes) > 500
    seen = set()
    for (M, N, K), lay in itertools.product(shapes, (NT, NN, TN)):
        want = lib.wf3d_gemm_ws_bytes(M, N, K, lay)
        assert want == G.ws_bytes(lay, M, N, K), (G.LAYOUT_NAMES[lay], M, N, K)
        r = G.route(lay, M, N, K)
        seen.add((r.kind, lay == TN, r.planned > 1))
    # the sweep itself sees every kind split and unsplit, so a wrong kind changes some answer
    assert seen >= {(k, t, s) for k in (MID, BIG) for t in (False, True) for s in (False, True)} | {(SMALL, False, False), (SMALL, False, True)}


def test_model_bounds_are_consistent():
    for c, r in ROUTES:
        assert sum(r.nks) == r.ktotal and min(r.nks) >= 1, c.name
        assert r.nbm * r.bm >= c.M > (r.nbm - 1) * r.bm and r.nbn * r.bn >= c.N > (r.nbn - 1) * r.bn, c.name
        nofit = c.route(ws_fits=False)
        assert nofit.ksplit == 1 and nofit.nks == (r.ktotal,) and nofit.combine == "none", c.name


def test_xcd_remap_model_is_a_bijection():
    """The model of the kernel's remap, not the kernel: the GPU test poisons the output to see the kernel's."""
    for nwg in list(range(1, 600)) + [4095, 4096, 4097]:
        assert sorted(G.xcd_vid(b, nwg) for b in range(nwg)) == list(range(nwg)), nwg


def test_cases_are_small():
    for c in G.CASES:
        assert max(c.M, c.N) <= 4096 and c.K <= 16384, c.name
        assert c.M * c.N * c.K <= 1.5e9, c.name


# ---- every named route has a case ------------------------------------------------------------------------------------
def _have(pred):
    return [c.name for c, r in ROUTES if pred(c, r)]


def _need(what, pred):
    assert _have(pred), f"no case reaches: {what}"


KIND_LAYOUT = [(SMALL, NT), (SMALL, NN), (MID, NT), (MID, NN), (MID, TN), (BIG, NT), (BIG, NN), (BIG, TN)]


def test_every_tile_kind_layout_and_arithmetic_has_a_case():
    for kind, lay in KIND_LAYOUT:
        _need((kind, lay, "fp32"), lambda c, r: (r.kind, c.layout) == (kind, lay) and not c.x3)
        if kind != SMALL:
            _need((kind, lay, "x3"), lambda c, r: (r.kind, c.layout) == (kind, lay) and r.x3)
        else:
            _need((kind, lay, "x3 asked, fp32 run"), lambda c, r: (r.kind, c.layout) == (kind, lay) and c.x3 and not r.x3)
    t128 = lambda c: G.cdiv(c.M, 128) * G.cdiv(c.N, 128)      # noqa: E731
    for x3 in (False, True):
        _need("TN big through N <= 64", lambda c, r: c.layout == TN and r.kind == BIG and c.N <= 64 < c.M and r.x3 == x3)
        _need("TN big through M <= 64", lambda c, r: c.layout == TN and r.kind == BIG and c.M <= 64 < c.N and r.x3 == x3)
        _need("TN big through t128 >= 64", lambda c, r: c.layout == TN and r.kind == BIG and min(c.M, c.N) > 64 and t128(c) >= 64
              and r.x3 == x3)
        _need("TN big through a long K", lambda c, r: c.layout == TN and r.kind == BIG and min(c.M, c.N) > 64 and t128(c) < 64
              and r.x3 == x3)


def test_every_body_selection_has_a_case():
    for kind, lay in KIND_LAYOUT:
        for body in ("all", "some", "none"):
            _need((kind, lay, body), lambda c, r: (r.kind, c.layout, r.body) == (kind, lay, body))
        if kind != SMALL:
            _need((kind, lay, "all", "x3"), lambda c, r: (r.kind, c.layout, r.body) == (kind, lay, "all") and r.x3)
    # one defect alone forces the checked body: the same case without it has FAST workgroups
    for what, field in (("lda % 4", "a_pad"), ("ldb % 4", "b_pad"), ("A base", "a_off"), ("B base", "b_off"), ("gamma/beta base", "p_off")):
        for lay in (NT, NN, TN):
            if field == "p_off" and lay == NN:
                continue

            def alone(c, r):
                if c.layout != lay or r.body != "none" or not getattr(c, field):
                    return False
                defects = [f for f in ("a_pad", "b_pad", "a_off", "b_off", "p_off") if getattr(c, f)]
                return defects == [field] and dataclasses.replace(c, **{field: 0}).route().body == "all"
            _need((what, lay), alone)
    # mixed: the M, N remainders the interior / edge split is tested at, per tile kind
    for kind in (SMALL, MID, BIG):
        bm, bn = G.TILE[kind]
        some = [(c, r) for c, r in ROUTES if r.kind == kind and r.body == "some" and r.ksplit == 1]
        assert {c.N % bn for c, _ in some} >= {1, 31, 33, bn - 1}, kind
        assert {c.M % bm for c, _ in some} >= ({1, 31} if bm == 32 else {1, 31, 33, bm - 1}), kind
        tails = {c.K % 32 for c, r in ROUTES if r.kind == kind and r.ksplit == 1 and c.M % bm == 0 and c.N % bn == 0}
        assert tails >= {1, 3, 29, 31}, kind
    for lay in (NT, NN, TN):
        _need(("K tail", lay, "x3"), lambda c, r: c.layout == lay and r.x3 and c.K % 32 in (1, 3, 29, 31))
        _need(("M/N edge", lay, "x3"), lambda c, r: c.layout == lay and r.x3 and r.body == "some")


def test_every_pipeline_depth_has_a_case():
    for R in (1, 2, 3):
        mine = [(c, r) for c, r in ROUTES if r.R == R]
        unsplit = {r.nks[0] for c, r in mine if r.ksplit == 1}
        assert unsplit >= {1, R, R + 1, 2 * R, 2 * R + 1}, (R, sorted(unsplit))
        assert any(r.ksplit == 1 and c.K % 32 and r.nks[0] > R for c, r in mine), f"R = {R}: no partial last slice past R slices"
        assert any(r.ksplit > 1 and c.K % 32 for c, r in mine), f"R = {R}: no split-K case whose last range alone is partial"
        # split-K ranges of both kinds: nk <= R and nk > R with nk % R != 0
        if R > 1:
            assert any(r.ksplit > 1 and max(r.nks) > R and max(r.nks) % R for c, r in mine), R
    _need("R = 3 on the 32-row tile", lambda c, r: r.R == 3 and r.kind == SMALL)
    _need("R = 3 on the 64x64 tile with a prologue", lambda c, r: r.R == 3 and r.kind == MID and c.pro is not None)


def test_every_workgroup_count_residue_has_a_case():
    counts = {r.nwg for c, r in ROUTES if r.ksplit == 1}
    assert counts >= set(range(1, 9)), sorted(counts)
    assert {n % 8 for n in counts if n > 8} == set(range(8)), sorted(counts)
    grids = {(r.nbm, r.nbn) for c, r in ROUTES}
    assert grids >= {(1, 7), (3, 3), (2, 5), (11, 1), (3, 4), (13, 1), (2, 7), (3, 5)}, sorted(grids)


def test_every_split_k_form_has_a_case():
    forms = {"2 narrow": lambda c, r: r.ksplit == 2 and r.combine == "narrow",
             "16 narrow": lambda c, r: r.ksplit == 16 and r.combine == "narrow",
             "17..31 wide": lambda c, r: 17 <= r.ksplit <= 31 and r.combine == "wide",
             "33..47 wide": lambda c, r: 33 <= r.ksplit <= 47 and r.combine == "wide",
             "49..63 wide": lambda c, r: 49 <= r.ksplit <= 63 and r.combine == "wide",
             "64 wide": lambda c, r: r.ksplit == 64 and r.combine == "wide",
             "> 64 wide": lambda c, r: r.ksplit > 64 and r.combine == "wide",
             "17..63, N % 4 != 0: narrow": lambda c, r: 17 <= r.ksplit <= 63 and c.N % 4 and r.combine == "narrow",
             ">= 64, N % 4 != 0: narrow": lambda c, r: r.ksplit >= 64 and c.N % 4 and r.combine == "narrow"}
    for what, f in forms.items():
        _need(what + ", every epilogue term", lambda c, r: f(c, r) and c.epilogue_all)
        _need(what + ", no epilogue term", lambda c, r: f(c, r) and c.epilogue_none)
    for kind, lay in KIND_LAYOUT:
        _need(("split", kind, lay), lambda c, r: (r.kind, c.layout) == (kind, lay) and r.ksplit > 1)
    _need("split x3 narrow", lambda c, r: r.x3 and r.combine == "narrow")
    _need("split x3 wide", lambda c, r: r.x3 and r.combine == "wide")


def test_every_epilogue_term_has_a_case():
    for kind in (SMALL, MID, BIG):
        _need(("bias alone", kind), lambda c, r: r.kind == kind and c.bias and not (c.addend >= 0 or c.accumulate or c.lr_k))
        _need(("addend, ld_addend > N", kind), lambda c, r: r.kind == kind and c.addend > 0 and r.ksplit == 1)
        _need(("accumulate, ldc > N", kind), lambda c, r: r.kind == kind and c.accumulate and c.ldc_pad > 0 and r.ksplit == 1)
        _need(("gap columns", kind), lambda c, r: r.kind == kind and c.ldc_pad > 0 and not c.accumulate)
    for k in (1, 2, 3, 4):
        _need(f"low-rank k = {k} in the kernel", lambda c, r: c.lr_k == k and c.lr_pad > 0 and r.ksplit == 1)
        _need(f"low-rank k = {k} through the narrow combine", lambda c, r: c.lr_k == k and c.lr_pad > 0 and r.combine == "narrow") \
            if k >= 3 else _need(f"low-rank k = {k} through the wide combine", lambda c, r: c.lr_k == k and c.lr_pad > 0 and r.combine == "wide")


def test_every_prologue_variant_has_a_case():
    for lay, kind in ((NT, SMALL), (NT, MID), (NT, BIG), (TN, MID), (TN, BIG)):
        for split in (False, True):
            mine = [(c, r) for c, r in ROUTES if c.pro is not None and (c.layout, r.kind, r.ksplit > 1) == (lay, kind, split)]
            got = {((c.pro.ln, c.pro.affine), c.pro.act) for c, _ in mine}
            want = {((False, False), G.ACT_RELU), ((False, False), G.ACT_GELU), ((True, False), G.ACT_NONE), ((False, True), G.ACT_NONE),
                    ((True, True), G.ACT_NONE), ((True, True), G.ACT_RELU), ((True, True), G.ACT_GELU)}
            assert got >= want, (lay, kind, split, sorted(want - got))
            assert {c.pro.drop for c, _ in mine} == {False, True}, (lay, kind, split)
            if kind != SMALL:
                assert any(r.x3 for _, r in mine), (lay, kind, split, "x3")
            assert any(c.pro.drop and c.pro.ln and c.pro.affine for c, _ in mine), (lay, kind, split, "dropout on LN + affine")
    _need("prologue + split + every epilogue term", lambda c, r: c.pro is not None and r.ksplit > 1 and c.epilogue_all)


def test_degenerate_and_production_calls_have_cases():
    for lay in (NT, NN, TN):
        for what, f in (("M = 1", lambda c: c.M == 1 and c.N > 1), ("N = 1", lambda c: c.N == 1 and c.M > 1),
                        ("K = 1", lambda c: c.K == 1 and c.M > 1), ("1 x 1 x 1", lambda c: (c.M, c.N, c.K) == (1, 1, 1))):
            _need((what, lay), lambda c, r: c.layout == lay and f(c))
    _need("K = 3 product at ldb = 1031, accumulate", lambda c, r: c.layout == NT and c.K == 3 and c.N + 0 and c.K + c.b_pad == 1031
          and c.accumulate)
    _need("low-rank V at stride 1031", lambda c, r: c.lr_k == 3 and c.lr_k + c.lr_pad == 1031)
    _need("N = 3 wgrad at ldc = 1031: big tile, split-K, no prologue",
          lambda c, r: c.layout == TN and c.N == 3 and c.N + c.ldc_pad == 1031 and r.kind == BIG and r.ksplit > 1 and c.pro is None)
    _need("N = 3 wgrad at ldc = 1031, one K range", lambda c, r: c.layout == TN and c.N == 3 and c.N + c.ldc_pad == 1031 and r.ksplit == 1)


# ---- the exact data sets are exact -------------------------------------------------------------------------------------
EXACT = [(c.name, ds) for c in G.CASES for ds in c.exact_sets()]


def _check_exact(case, ds):
    inp = G.inputs(case, ds)
    # every partial sum, in any order, is an fp32 number
    assert G.grid_units(case, inp) < 2 ** 24, "partial sums leave the fp32 grid"
    # the prologue is exact in fp32
    if case.pro is not None:
        h32, h64 = G.prologue32(case, inp), G.prologue64(case, inp, True)
        assert np.array_equal(h32.astype(np.float64), h64), "prologue inexact in fp32"
        if case.pro.act == G.ACT_GELU:
            # the GELU-as-ReLU premise: no pre-activation strictly between -8 and 8 but zero
            pre = G.prologue64(_without_act(case), {k: v for k, v in inp.items() if k != "drop"}, True)
            assert np.all((pre == 0) | (np.abs(pre) >= 8)), "a GELU argument inside (-8, 8)"
    # the reference is its own fp32 rounding
    ref, _, extra = G.reference(case, inp, True)
    assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref) and not extra.any()
    if ds in ("x3a", "x3b"):
        P, Q = G.operands64(case, inp, True)
        (ph, pl), (qh, ql) = sx8_model.split(P.astype(np.float32)), sx8_model.split(Q.astype(np.float32))
        big, small = ((ph, pl), (qh, ql)) if ds == "x3a" else ((qh, ql), (ph, pl))
        src = (P if ds == "x3a" else Q)
        live = src != 0
        assert np.array_equal(big[0].astype(np.float64) + big[1].astype(np.float64), src), "hi + lo is not the value"
        assert np.all(big[1][live] != 0) and np.all(big[0][live] != 0), "a dead plane on the 16-bit operand"
        assert not small[1].any(), "the small operand has a low part"
        # so ah.bh + al.bh (x3a) / ah.bh + ah.bl (x3b) is the product, and each of the two terms is needed
        assert live.mean() > 0.2 or case.pro is not None
    elif case.route().x3:
        P, Q = G.operands64(case, inp, True)
        assert not sx8_model.split(P.astype(np.float32))[1].any() and not sx8_model.split(Q.astype(np.float32))[1].any()


def _without_act(case):
    return dataclasses.replace(case, pro=dataclasses.replace(case.pro, act=G.ACT_NONE, drop=False))


@pytest.mark.parametrize("ds", G.DATA_EXACT)
def test_exact_data_sets_are_exact(ds):
    n = 0
    for c in G.CASES:
        if ds in c.exact_sets():
            try:
                _check_exact(c, ds)
            except AssertionError as e:
                raise AssertionError(f"{c.name} / {ds}: {e}") from e
            n += 1
    assert n >= (300 if ds == "int" else 60)


def test_gelu_saturates_in_fp32_where_the_exact_sets_put_it():
    """The kernel's erf (csrc/wf3d_common.h, wf3d_erf) in numpy float32: at |y| >= 8 it returns +-1 exactly, so GELU(y) is y
    or -0: on the exact sets a GELU prologue is a ReLU bit for bit."""
    f = np.float32
    y = np.concatenate([np.arange(8, 4096, 8), 2.0 ** np.arange(3, 20), 65535.0 * np.arange(1, 5)]).astype(f)
    a = y * f(0.70710678118654752440)
    t, s = np.abs(a), a * a
    r = f(-1.72853470e-5) * t + f(3.83197126e-4)
    u = f(-3.88396438e-3) * t + f(2.42546219e-2)
    r = r * s + u
    for cst in (-1.06777877e-1, -6.34846687e-1, -1.28717512e-1):
        r = r * t + f(cst)
    r = r * t - t
    assert r.dtype == np.float32 and np.all(r < -17.4)          # exp(r) < 2^-25: 1 - exp(r) rounds to 1 in any rounding of exp
    with np.errstate(under="ignore", over="ignore"):
        assert np.all(f(1) - np.exp(r) == f(1))
