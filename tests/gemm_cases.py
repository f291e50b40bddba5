"""Route model, case table and data of the general fp32 / bf16x3 GEMM (wf3d_gemm, csrc/gemm.hip).

TEST INFRASTRUCTURE ONLY.  Three parts, all plain Python + numpy (no GPU, no library):

    route(layout, M, N, K, ...)   the host-side decisions of wf3d_gemm restated from its code: tile kind, block grid,
                                  split-K plan, register sets R, K slices per range, combine kind, and how many
                                  workgroups take the branch-free FAST body.  tests/test_gemm_cases.py holds it to
                                  wf3d_gemm_ws_bytes; DESIGN.md "wf3d_gemm: routes" is its prose.
    CASES                         named cases, each there for one route (`why`); the smallest shapes that reach it
    inputs(case, data)            the operands of a case as float32 numpy arrays, for the data sets
                                      "int"            small integers: every fp32 partial sum is exact
                                      "x3a" / "x3b"    bf16x3-exact: one operand holds 16-significant-bit values (hi and
                                                       lo plane both live, lo exactly a bf16), the other values in
                                                       {-2..2}; a = A is the 16-bit one, b = B
                                      "gauss"          standard normal
                                      "offset"         normal rows on a large common offset
    reference(case, inp)          (ref, S, extra) in float64: the result, the magnitude sum S_ij the error bounds scale
                                  with, and the absolute GELU allowance (zero without a GELU prologue)

Operands are stored as the kernel reads them: NT a[M,K] b[N,K]; NN a[M,K] b[K,N]; TN a[K,M] b[K,N].  The prologue acts on
the activation operand: A under NT (rows M, columns K), B under TN (rows K, columns N).
"""
import dataclasses
import zlib

import numpy as np
import torch

from oracle import dropout as D

NT, NN, TN = 0, 1, 2
LAYOUT_NAMES = ("NT", "NN", "TN")
ACT_NONE, ACT_RELU, ACT_GELU = 0, 1, 2
BK = 32
SMALL, MID, BIG = "32x128", "64x64", "128x128"
TILE = {SMALL: (32, 128), MID: (64, 64), BIG: (128, 128)}


def cdiv(a, b):
    return -(-a // b)


# ---- the route model ---------------------------------------------------------------------------------------------
# WF3D_SPLITK_GEMM (csrc/wf3d_common.h): nosplit_tiles, target, cap, few_tiles, few_slices, few_cap, few_mult8
SPLITK_GEMM = (256, 512, 64, 8, 4, 256, False)


def splitk_plan(tiles, ktotal, rule=SPLITK_GEMM):
    """(ksplit, kt_per) of wf3d_splitk_plan with rounds = 1."""
    nosplit, target, cap, few_tiles, few_slices, few_cap, few_mult8 = rule
    if tiles >= nosplit or ktotal < 8:
        return 1, ktotal
    few = tiles <= few_tiles
    want = cdiv(target, tiles)
    most = ktotal // (few_slices if few else 4)
    ks = min(want, most, few_cap if few else cap)
    if few and few_mult8 and ks >= 8:
        ks &= ~7
    if ks < 2:
        return 1, ktotal
    kt_per = cdiv(ktotal, ks)
    return cdiv(ktotal, kt_per), kt_per


def tile_kind(layout, M, N, K):
    t128 = cdiv(M, 128) * cdiv(N, 128)
    t64 = cdiv(M, 64) * cdiv(N, 64)
    if layout != TN:
        if M <= 64:
            return SMALL
        return MID if (t128 < 256 and t64 >= 128 and K <= 2048) else BIG
    return MID if (M > 64 and N > 64 and t128 < 64 and (K <= 4096 or t128 <= 16)) else BIG


@dataclasses.dataclass(frozen=True)
class Route:
    kind: str
    bm: int
    bn: int
    nbm: int
    nbn: int
    ktotal: int
    ksplit: int           # after the workspace fit
    planned: int          # what the planner asked for (enters wf3d_gemm_ws_bytes)
    kt_per: int
    R: int
    x3: bool              # the arithmetic that runs (x3 asked for on the 32-row tile runs fp32)
    nks: tuple            # K slices of each K range
    combine: str          # "none", "narrow" or "wide"
    body: str             # "all", "some" or "none" of the workgroups take the FAST body
    n_fast: int
    k_partial: bool       # the last K slice is partial

    @property
    def nwg(self):
        return self.nbm * self.nbn


def route(layout, M, N, K, x3=False, pro=False, vecA=True, vecB=True, vecP=True, ws_fits=True):
    kind = tile_kind(layout, M, N, K)
    bm, bn = TILE[kind]
    nbm, nbn = cdiv(M, bm), cdiv(N, bn)
    ktotal = cdiv(K, BK)
    planned, kt_per = splitk_plan(nbm * nbn, ktotal)
    ksplit = planned
    if not ws_fits:
        ksplit, kt_per = 1, ktotal
    R = 3 if kind != BIG else (1 if pro else 2)
    ranges = [(z * kt_per, min(ktotal, (z + 1) * kt_per)) for z in range(ksplit)]
    n_fast = 0
    if vecA and vecB and vecP:
        full_m, full_n = M // bm, N // bn           # tiles wholly inside the matrix
        n_fast = full_m * full_n * sum(1 for _, kt1 in ranges if kt1 * BK <= K)
    total = nbm * nbn * ksplit
    return Route(kind=kind, bm=bm, bn=bn, nbm=nbm, nbn=nbn, ktotal=ktotal, ksplit=ksplit, planned=planned, kt_per=kt_per, R=R,
                 x3=bool(x3) and kind != SMALL, nks=tuple(b - a for a, b in ranges),
                 combine="none" if ksplit == 1 else ("wide" if ksplit > 16 and N % 4 == 0 else "narrow"),
                 body="all" if n_fast == total else ("some" if n_fast else "none"), n_fast=n_fast, k_partial=K % BK != 0)


def ws_bytes(layout, M, N, K):
    """wf3d_gemm_ws_bytes: the planner's slabs."""
    r = route(layout, M, N, K)
    return r.planned * M * N * 4 if r.planned > 1 else 0


def xcd_vid(bid, nwg):
    """The kernel's tile of workgroup `bid`: workgroups bid, bid + 8, ... share an XCD and get consecutive tiles."""
    q, r, xcd = nwg >> 3, nwg & 7, bid & 7
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + (bid >> 3)


# ---- cases ---------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Pro:
    ln: bool = False
    affine: bool = False
    act: int = ACT_NONE
    drop: bool = False

    @property
    def variant(self):
        base = {(False, False): "act", (True, False): "ln", (False, True): "affine", (True, True): "ln+affine"}[(self.ln, self.affine)]
        return base + ":" + ("none", "relu", "gelu")[self.act] + (":drop" if self.drop else "")


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    why: str
    layout: int
    M: int
    N: int
    K: int
    x3: bool = False
    pro: Pro = None
    bias: bool = False
    addend: int = -1          # -1: none; else extra columns of the addend's rows (ld_addend = N + addend)
    accumulate: bool = False
    ldc_pad: int = 0          # extra columns of the output's rows
    lr_k: int = 0             # low-rank term U[M,k] V[N,k]^T
    lr_pad: int = 0           # extra columns of U's and V's rows
    a_pad: int = 0            # extra columns of A's / B's stored rows
    b_pad: int = 0
    a_off: int = 0            # floats between a 16-B boundary and the operand's first element
    b_off: int = 0
    p_off: int = 0            # the same for gamma and beta

    def a_shape(self):
        return (self.M, self.K) if self.layout != TN else (self.K, self.M)

    def b_shape(self):
        return (self.N, self.K) if self.layout == NT else (self.K, self.N)

    def ld(self, shape, pad):
        """ops.gemm's rule: a single stored row has its length as leading dimension."""
        return shape[1] + pad if shape[0] > 1 else max(shape[1], 1)

    def route(self, ws_fits=True):
        affine = self.pro is not None and self.pro.affine
        return route(self.layout, self.M, self.N, self.K, x3=self.x3, pro=self.pro is not None,
                     vecA=self.a_off % 4 == 0 and self.ld(self.a_shape(), self.a_pad) % 4 == 0,
                     vecB=self.b_off % 4 == 0 and self.ld(self.b_shape(), self.b_pad) % 4 == 0,
                     vecP=not affine or self.p_off % 4 == 0, ws_fits=ws_fits)

    @property
    def epilogue_all(self):
        return self.bias and self.addend >= 0 and self.accumulate and self.lr_k > 0

    @property
    def epilogue_none(self):
        return not (self.bias or self.addend >= 0 or self.accumulate or self.lr_k)

    def exact_sets(self):
        return ("int", "x3a", "x3b") if self.route().x3 else ("int",)


ALL_EPI = dict(bias=True, addend=5, accumulate=True, ldc_pad=7, lr_k=3, lr_pad=2)
CASES = []


def _add(name, why, layout, M, N, K, **kw):
    CASES.append(Case(name, why, layout, M, N, K, **kw))


def _vec_pads(layout, M, N):
    """Row padding that keeps the row-contiguous operands 16-B loadable when M or N is no multiple of 4."""
    return dict(a_pad=-M % 4 if layout == TN else 0, b_pad=-N % 4 if layout != NT else 0)


def _build():
    L = LAYOUT_NAMES
    # -- tile kind x layout, x3 on and off (x3 on the 32-row tile runs fp32 by design)
    for lay in (NT, NN):
        for x3 in (False, True):
            t = f"{L[lay]}{'_x3' if x3 else ''}"
            _add(f"kind_small_{t}", "32x128 tile" + (", x3 asked for: runs fp32" if x3 else ""), lay, 40, 200, 96, x3=x3, bias=True)
            _add(f"kind_mid_{t}", "64x64 tile", lay, 449, 991, 96, x3=x3, bias=True)
            _add(f"kind_big_{t}", "128x128 tile", lay, 161, 257, 96, x3=x3, bias=True)
    for x3 in (False, True):
        t = "TN_x3" if x3 else "TN"
        _add(f"kind_mid_{t}", "TN 64x64 tile (tn_mid)", TN, 130, 190, 96, x3=x3)
        _add(f"kind_big_{t}_narrowN", "TN 128x128 through N <= 64", TN, 200, 64, 96, x3=x3)
        _add(f"kind_big_{t}_shortM", "TN 128x128 through M <= 64", TN, 64, 200, 96, x3=x3)
        _add(f"kind_big_{t}_t128", "TN 128x128 through t128 >= 64", TN, 1000, 1024, 40, x3=x3)
        _add(f"kind_big_{t}_longK", "TN 128x128 through K > 4096 with t128 > 16", TN, 520, 500, 4100, x3=x3)

    # -- body selection
    for lay, kind, (M, N) in ((NT, "small", (64, 256)), (NN, "small", (32, 128)), (NT, "mid", (512, 1024)), (NN, "mid", (512, 1024)),
                              (TN, "mid", (128, 192)), (NT, "big", (256, 128)), (NN, "big", (128, 256))):
        for x3 in ((False, True) if kind != "small" else (False,)):
            _add(f"fast_all_{kind}_{L[lay]}{'_x3' if x3 else ''}", "every workgroup FAST: aligned, whole tiles", lay, M, N, 128, x3=x3)
    _add("fast_all_big_TN", "every workgroup FAST on the TN big tile (t128 >= 64)", TN, 1024, 1024, 64)
    _add("fast_all_big_TN_x3", "every workgroup FAST on the TN big tile, x3", TN, 1024, 1024, 64, x3=True)
    for lay, (M, N) in ((NT, (256, 128)), (NN, (256, 128)), (TN, (128, 192))):
        t = L[lay]
        _add(f"slow_lda_{t}", "lda % 4 != 0 alone forces the checked body", lay, M, N, 64, a_pad=1)
        _add(f"slow_ldb_{t}", "ldb % 4 != 0 alone forces the checked body", lay, M, N, 64, b_pad=3)
        _add(f"slow_abase_{t}", "A one float off a 16-B boundary alone forces the checked body", lay, M, N, 64, a_off=1)
        _add(f"slow_bbase_{t}", "B one float off a 16-B boundary alone forces the checked body", lay, M, N, 64, b_off=1, x3=True)
    _add("slow_gamma_NT", "gamma/beta one float off alone forces the checked body", NT, 256, 128, 64,
         pro=Pro(True, True, ACT_RELU), p_off=1)
    _add("slow_gamma_NT_mid", "gamma/beta one float off, 64x64 tile", NT, 512, 1024, 64, pro=Pro(False, True, ACT_NONE), p_off=1)
    _add("slow_gamma_TN", "gamma/beta one float off, TN", TN, 128, 192, 64, pro=Pro(True, True, ACT_RELU), p_off=1)
    # mixed: interior workgroups FAST, edge ones checked; M, N remainders 1, 31, 33, tile - 1
    for i, (rm, rn) in enumerate(((1, 31), (31, 33), (33, -1), (-1, 1))):
        for lay, kind, (bm, bn), (tm, tn) in ((NT, "small", (32, 128), (1, 2)), (NN, "small", (32, 128), (1, 1)),
                                               (NT, "mid", (64, 64), (7, 15)), (NN, "mid", (64, 64), (15, 7)),
                                               (TN, "mid", (64, 64), (2, 1)), (NT, "big", (128, 128), (1, 2)),
                                               (NN, "big", (128, 128), (2, 1)), (TN, "big", (128, 128), (7, 8))):
            M = tm * bm + (rm if rm > 0 else bm - 1)
            N = tn * bn + (rn if rn > 0 else bn - 1)
            if kind == "small":
                M = 33 if i % 2 == 0 else 63                # M <= 64: one whole 32-row tile and a remainder of 1 or 31
            x3 = kind != "small" and i % 2 == 1
            _add(f"mixed_{kind}_{L[lay]}_{i}", f"interior FAST, edges checked: M = {M}, N = {N}", lay, M, N, 64, x3=x3,
                 bias=(i == 0), **_vec_pads(lay, M, N))
    # K remainders within the last slice: no workgroup FAST without split-K
    for i, rk in enumerate((1, 3, 29, 31)):
        for lay, kind, (M, N) in ((NT, "small", (64, 128)), (NN, "mid", (512, 1024)), (TN, "mid", (128, 128)),
                                  (NT, "big", (128, 128)), (TN, "big", (64, 128)), (NN, "big", (128, 128))):
            x3 = bool((i + lay) % 2) and kind != "small"
            _add(f"ktail_{kind}_{L[lay]}_{rk}", f"K = 64 + {rk}: zero-fill of the last slice", lay, M, N, 64 + rk, x3=x3)

    # -- pipeline: nk against R
    for R, lay, (M, N), pro in ((3, NT, (64, 128), None), (3, TN, (128, 128), None), (3, NT, (512, 1024), Pro(True, True, ACT_RELU)),
                                (2, NT, (128, 128), None), (2, TN, (64, 128), None), (2, NN, (256, 128), None),
                                (1, NT, (128, 128), Pro(True, True, ACT_RELU)), (1, TN, (64, 128), Pro(True, True, ACT_RELU))):
        for nk in sorted({1, R, R + 1, 2 * R, 2 * R + 1}):
            x3 = lay != NT and nk % 2 == 0 and not (lay == NN and M <= 64)
            _add(f"pipe_R{R}_{L[lay]}{'_pro' if pro else ''}_nk{nk}", f"R = {R}, {nk} slices", lay, M, N, 32 * nk, pro=pro, x3=x3)
        # a partial last slice at nk = R + 1 (the clamped fetch re-reads it)
        _add(f"pipe_R{R}_{L[lay]}{'_pro' if pro else ''}_partial", f"R = {R}, {R + 1} slices, the last one partial", lay, M, N,
             32 * R + 13, pro=pro)

    # -- XCD remap: nbm x nbn workgroups of every residue mod 8 (output starts as NaN poison in every case)
    for nm, lay, M, N in (("1x7", NT, 20, 7 * 128 - 5), ("3x3", NT, 300, 300), ("2x5", TN, 100, 300), ("11x1", NT, 1300, 100),
                          ("3x4", TN, 190, 250), ("13x1", NN, 1600, 50), ("2x7", NN, 40, 800), ("3x5", TN, 170, 290),
                          ("2x4", TN, 128, 256), ("2x8", NN, 64, 1024), ("1x1", NT, 100, 100), ("1x2", NT, 100, 200),
                          ("1x3", NN, 30, 300), ("2x2", TN, 100, 100), ("5x1", NT, 600, 100), ("2x3", TN, 250, 300),
                          ("5x5", NT, 600, 600), ("9x2", NN, 1100, 250), ("1x25", NT, 10, 3100)):
        _add(f"xcd_{nm}", f"XCD remap over {nm} workgroups", lay, M, N, 40)

    # -- split-K: each form with every epilogue term and with none
    for nm, lay, M, N, K, why in (("ks2", NT, 64, 128, 256, "2 ranges, narrow"),
                                  ("ks2_tail", NN, 200, 100, 300, "2 ranges, only the last partial"),
                                  ("ks16", TN, 128, 128, 2048, "16 ranges, narrow"),
                                  ("ks17", NT, 64, 128, 2176, "17 ranges, wide"),
                                  ("ks17_N3", TN, 200, 3, 2176, "17 ranges, N % 4 != 0: narrow"),
                                  ("ks23", NN, 130, 132, 2944, "23 ranges, wide"),
                                  ("ks37", TN, 128, 64, 4736, "37 ranges, wide"),
                                  ("ks63", NT, 150, 60, 8064 - 5, "63 ranges, wide, last range partial"),
                                  ("ks64", TN, 256, 8, 8192, "64 ranges, wide"),
                                  ("ks80", NT, 33, 100, 10240, "80 ranges, wide: a second pass of the slab loop"),
                                  ("ks64_N6", NN, 64, 6, 8192, "64 ranges, N % 4 != 0: narrow")):
        _add(f"split_{nm}_plain", why + "; no epilogue term", lay, M, N, K)
        _add(f"split_{nm}_epi", why + "; every epilogue term", lay, M, N, K, **ALL_EPI)
    _add("split_ks16_x3", "16 ranges in x3, TN 64x64", TN, 128, 128, 2048, x3=True)
    _add("split_ks17_x3_epi", "17 ranges in x3, big tile, every epilogue term", NT, 100, 128, 2176, x3=True, **ALL_EPI)
    _add("split_mid_NT", "64x64 tile with 2 ranges (128 tiles)", NT, 512, 1024, 256)
    _add("split_mid_NN", "64x64 tile with 2 ranges, NN", NN, 512, 1024, 256 + 3)
    _add("split_mid_NT_x3_epi", "64x64 tile with 2 ranges in x3, every epilogue term", NT, 512, 1024, 256 + 17, x3=True, **ALL_EPI)

    # -- epilogue terms one at a time, and the low-rank term k = 1..4, in-kernel and through the combine
    for lay, M, N, K, t in ((NT, 40, 130, 40, "small"), (TN, 130, 70, 40, "mid"), (NN, 130, 70, 40, "big")):
        _add(f"epi_bias_{t}", "bias alone", lay, M, N, K, bias=True)
        _add(f"epi_addend_{t}", "addend with ld_addend > N", lay, M, N, K, addend=9)
        _add(f"epi_acc_{t}", "accumulate into a strided out", lay, M, N, K, accumulate=True, ldc_pad=11)
        _add(f"epi_gap_{t}", "strided out without accumulate: gap columns stay", lay, M, N, K, ldc_pad=3)
    for k in (1, 2, 3, 4):
        _add(f"epi_lr{k}_kernel", f"low-rank k = {k} in the kernel, strided U and V", (NT, TN, NN, NT)[k - 1], 130, 70, 40, lr_k=k,
             lr_pad=k, x3=(k % 2 == 0))
        _add(f"epi_lr{k}_combine", f"low-rank k = {k} through the combine", (NT, TN, NN, NT)[k - 1], 130, 72 if k < 3 else 70, 2176,
             lr_k=k, lr_pad=5 - k)

    # -- prologue variants on every tile kind that has them, and under split-K
    variants = [Pro(False, False, ACT_RELU), Pro(False, False, ACT_GELU), Pro(True, False, ACT_NONE), Pro(False, True, ACT_NONE),
                Pro(True, True, ACT_NONE), Pro(True, True, ACT_RELU), Pro(True, True, ACT_GELU)]
    places = (("NT_small", NT, 50, 130, 70), ("NT_mid", NT, 449, 991, 70), ("NT_big", NT, 161, 130, 70),
              ("TN_mid", TN, 130, 100, 70), ("TN_big", TN, 60, 130, 70),
              ("NT_small_split", NT, 50, 130, 300), ("NT_big_split", NT, 161, 132, 2176 + 9),
              ("TN_mid_split", TN, 130, 100, 300), ("TN_big_split", TN, 60, 132, 2176 + 9), ("NT_mid_split", NT, 449, 991, 256))
    for pi, (pn, lay, M, N, K) in enumerate(places):
        for vi, v in enumerate(variants):
            for drop in (False, True):
                if drop and (vi + pi) % 2:          # dropout on half of the variants of each place, alternating
                    continue
                x3 = "small" not in pn and (vi + pi) % 3 == 0
                pv = dataclasses.replace(v, drop=drop)
                epi = ALL_EPI if (drop and "split" in pn and vi >= 4) else {}
                _add(f"pro_{pn}_{pv.variant.replace(':', '_').replace('+', '')}{'_x3' if x3 else ''}",
                     f"prologue {pv.variant} on {pn}", lay, M, N, K, pro=pv, x3=x3, **epi)

    # -- degenerate dimensions and the production K = 3 / N = 3 calls at their own stride (1031 = 2 * 512 + 2 * 3 + 1)
    for lay in (NT, NN, TN):
        t = L[lay]
        _add(f"deg_M1_{t}", "M = 1", lay, 1, 70, 40, bias=True)
        _add(f"deg_N1_{t}", "N = 1", lay, 70, 1, 40, bias=True)
        _add(f"deg_K1_{t}", "K = 1", lay, 70, 40, 1, bias=True)
        _add(f"deg_111_{t}", "M = N = K = 1", lay, 1, 1, 1)
    _add("deg_N1_split", "N = 1 with a long K (TN wgrad of a bias-like column)", TN, 257, 1, 2048)
    _add("prod_K3_NT_acc", "coordinate product cv . Wc^T into Pa: K = 3, ldb = 1031, accumulate", NT, 300, 512, 3, b_pad=1028,
         accumulate=True)
    _add("prod_K3_lowrank", "the same product as the low-rank term of the in-projection (V at stride 1031)", NT, 300, 512, 64, x3=True,
         bias=True, lr_k=3, lr_pad=1028)
    _add("prod_K3_NN", "dcv += dza . P0w: N = 3, accumulate", NN, 300, 3, 512, accumulate=True)
    _add("prod_N3_wgrad", "wgrad dPa^T . cv into dW0[:, 2H:2H+3]: N = 3, ldc = 1031, big tile, split-K", TN, 512, 3, 2176, ldc_pad=1028)
    _add("prod_N3_wgrad_short", "the same wgrad over few rows: one K range", TN, 512, 3, 200, ldc_pad=1028)


_build()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES), "duplicate case names"


# ---- data ------------------------------------------------------------------------------------------------------------
DATA_EXACT = ("int", "x3a", "x3b")
DATA_GENERAL = ("gauss", "offset")
DROP_P = {"int": 0.5, "x3a": 0.5, "x3b": 0.5, "gauss": 0.1, "offset": 0.3}
X3_BUDGET = 0.75 * 2 ** 24       # sum_k |a||b| allowed on the x3 sets, in grid units; the epilogue terms take the rest
OFFSET = 1000.0


def _rng(case, data, what):
    return np.random.default_rng(zlib.crc32(f"{case.name}/{data}/{what}".encode()))


def _ints(rng, shape, lo, hi, nonzero=False):
    v = rng.integers(lo, hi + 1, size=shape)
    if nonzero:
        v = np.where(v == 0, hi, v)
    return v.astype(np.float32)


def _big16(rng, shape):
    """+-(256 H + L), H in 128..255, L in 1..255 except 128: 16 significant bits, hi = bf16 rounding down (L < 128) or up
    (L > 128), lo = L or L - 256: both planes non-zero, both exactly bf16."""
    H = rng.integers(128, 256, size=shape)
    Lw = rng.integers(1, 255, size=shape)
    Lw = np.where(Lw >= 128, Lw + 1, Lw)
    s = rng.integers(0, 2, size=shape) * 2 - 1
    return (s * (256 * H + Lw)).astype(np.float32)


def _sparse_small(rng, shape, k_axis, peak):
    """Values in {-2..2} \\ {0} at so many places along K per line that sum_k |16-bit value| * peak stays inside X3_BUDGET
    (peak: the largest magnitude the prologue can make of a 2), always including k = 0 and k = K - 1."""
    v = _ints(rng, shape, -2, 2, nonzero=True)
    K = shape[k_axis]
    NNZ = max(2, int(X3_BUDGET // (65535 * peak)))
    if K <= NNZ:
        return v
    lines = shape[1 - k_axis]
    keep = np.zeros((lines, K), dtype=bool)
    for i in range(lines):
        keep[i, rng.choice(K, NNZ - 2, replace=False)] = True
    keep[:, 0] = keep[:, K - 1] = True
    return np.where(keep if k_axis == 1 else keep.T, v, np.float32(0))


def inputs(case, data):
    """dict of float32 arrays: A, B as stored; bias [N], addend [M,N], C0 [M,N], U [M,k], V [N,k]; mu, rs [rows]; gamma, beta
    [cols]; drop = (p, seed) — each present only where the case has the term."""
    c, p = case, case.pro
    exact = data in DATA_EXACT
    gelu = p is not None and p.act == ACT_GELU
    # exact data under GELU: every pre-activation is a multiple of 8, where the fp32 erf has saturated (GELU = ReLU bit for bit)
    sc = np.float32(8 if (exact and gelu) else 1)
    a_k, b_k = (1 if c.layout != TN else 0), (1 if c.layout == NT else 0)      # the K axis of each stored operand
    out = {}
    peak = 2 * (float(sc) if p is not None else 1) * (2 if p is not None and p.drop else 1) * (2 if p is not None else 1)
    ra, rb = _rng(c, data, "A"), _rng(c, data, "B")
    if data == "int":
        A, B = _ints(ra, c.a_shape(), -3, 3), _ints(rb, c.b_shape(), -3, 3)
    elif data == "x3a":
        A, B = _big16(ra, c.a_shape()), _sparse_small(rb, c.b_shape(), b_k, peak)
    elif data == "x3b":
        A, B = _sparse_small(ra, c.a_shape(), a_k, peak), _big16(rb, c.b_shape())
    else:
        A = ra.standard_normal(c.a_shape()).astype(np.float32)
        B = rb.standard_normal(c.b_shape()).astype(np.float32)
        if data == "offset":
            # the rows of the activation operand (A's logical rows without a prologue) ride on a large common offset
            tgt, axis = (B, 1) if (p is not None and c.layout == TN) else (A, a_k)
            off = (OFFSET * (1 + _rng(c, data, "off").random(tgt.shape[1 - axis]))).astype(np.float32)
            tgt += off[:, None] if axis == 1 else off[None, :]
    if p is not None:
        act_is_a = c.layout == NT
        X = A if act_is_a else B
        rows, cols = X.shape
        r = _rng(c, data, "pro")
        if data == "int":
            # integer mu, power-of-two rs, small-integer gamma and beta: every step of pro_one is exact in fp32
            X *= sc
            if p.ln:
                out["mu"] = _ints(r, rows, -2, 2) * sc
                out["rs"] = np.float32(2.0) ** r.integers(0 if gelu else -1, 2, size=rows).astype(np.float32)
            if p.affine:
                out["gamma"] = _ints(r, cols, -2, 2, nonzero=True)
                out["beta"] = _ints(r, cols, -2, 2) * sc
        elif exact:
            # x3 sets: the prologue keeps every operand bit and every zero (mu = 0, rs = 1, gamma = +-1, beta = 0), so the
            # 16-bit operand stays 16-bit and the sparse one sparse; its full arithmetic is the "int" set's business
            if data != ("x3a" if act_is_a else "x3b"):
                X *= sc
            if p.ln:
                out["mu"], out["rs"] = np.zeros(rows, np.float32), np.ones(rows, np.float32)
            if p.affine:
                out["gamma"] = (r.integers(0, 2, size=cols) * 2 - 1).astype(np.float32)
                out["beta"] = np.zeros(cols, np.float32)
        else:
            if p.ln:
                x64 = X.astype(np.float64)
                out["mu"] = x64.mean(1).astype(np.float32)
                out["rs"] = (1.0 / np.sqrt(x64.var(1) + 1e-5)).astype(np.float32)
            if p.affine:
                out["gamma"] = (1 + 0.5 * r.standard_normal(cols)).astype(np.float32)
                out["beta"] = (0.5 * r.standard_normal(cols)).astype(np.float32)
        if p.drop:
            out["drop"] = (DROP_P[data], int(r.integers(1, 2 ** 32)))
    out["A"], out["B"] = A, B
    e = _rng(c, data, "epi")
    gen = (lambda shape: _ints(e, shape, -3, 3)) if exact else (lambda shape: e.standard_normal(shape).astype(np.float32))
    if c.bias:
        out["bias"] = gen((c.N,))
    if c.addend >= 0:
        out["addend"] = gen((c.M, c.N))
    if c.accumulate:
        out["C0"] = gen((c.M, c.N))
    if c.lr_k:
        out["U"], out["V"] = gen((c.M, c.lr_k)), gen((c.N, c.lr_k))
    return out


def prologue64(case, inp, exact):
    """The activation operand after the prologue, float64 [rows, cols].  exact: GELU is taken as ReLU (see inputs)."""
    p = case.pro
    X = (inp["A"] if case.layout == NT else inp["B"]).astype(np.float64)
    if p is None:
        return X
    h = X
    if p.ln:
        h = (h - inp["mu"].astype(np.float64)[:, None]) * inp["rs"].astype(np.float64)[:, None]
    if p.affine:
        h = h * inp["gamma"].astype(np.float64)[None, :] + inp["beta"].astype(np.float64)[None, :]
    if p.act == ACT_RELU or (p.act == ACT_GELU and exact):
        h = np.maximum(h, 0.0)
    elif p.act == ACT_GELU:
        h = 0.5 * h * (1.0 + torch.erf(torch.from_numpy(h / np.sqrt(2.0))).numpy())
    if p.drop:
        pd, seed = inp["drop"]
        h = h * D.scaled(seed, np.arange(h.shape[0])[:, None], np.arange(h.shape[1])[None, :], pd)
    return h


def prologue32(case, inp):
    """The same in float32 operation by operation, as the kernel's pro_one (exact data only: GELU taken as ReLU)."""
    p = case.pro
    X = inp["A"] if case.layout == NT else inp["B"]
    if p is None:
        return X
    h = X
    if p.ln:
        h = (h - inp["mu"][:, None]) * inp["rs"][:, None]
    if p.affine:
        h = h * inp["gamma"][None, :] + inp["beta"][None, :]
    if p.act != ACT_NONE:
        h = np.maximum(h, np.float32(0))
    if p.drop:
        pd, seed = inp["drop"]
        h = h * D.scaled(seed, np.arange(h.shape[0])[:, None], np.arange(h.shape[1])[None, :], pd, dtype=np.float32)
    assert h.dtype == np.float32
    return h


def operands64(case, inp, exact):
    """(P [M,K], Q [K,N]) in float64: the two factors after the prologue, in the product's orientation."""
    h = prologue64(case, inp, exact)
    if case.layout == NT:
        return h, inp["B"].astype(np.float64).T
    if case.layout == NN:
        return inp["A"].astype(np.float64), inp["B"].astype(np.float64)
    return inp["A"].astype(np.float64).T, h


def reference(case, inp, exact):
    """(ref, S, extra): C in float64, S_ij = sum_k |p_ik||q_kj| + |bias_j| + sum |u||v| + |addend_ij| + |C0_ij|, and the
    absolute allowance of a GELU prologue, 2e-5 max|h| sum_k |other operand| (zero otherwise)."""
    P, Q = operands64(case, inp, exact)
    ref, S = P @ Q, np.abs(P) @ np.abs(Q)
    for k, f in (("bias", lambda t: t[None, :]), ("addend", lambda t: t), ("C0", lambda t: t)):
        if k in inp:
            t = f(inp[k].astype(np.float64))
            ref, S = ref + t, S + np.abs(t)
    if "U" in inp:
        U, V = inp["U"].astype(np.float64), inp["V"].astype(np.float64)
        ref, S = ref + U @ V.T, S + np.abs(U) @ np.abs(V).T
    extra = np.zeros_like(ref)
    if case.pro is not None and case.pro.act == ACT_GELU and not exact:
        if case.layout == NT:
            extra = extra + 2e-5 * np.abs(P).max() * np.abs(Q).sum(0)[None, :]
        else:
            extra = extra + 2e-5 * np.abs(Q).max() * np.abs(P).sum(1)[:, None]
    return ref, S, extra


def unit_roundoff_bound(case):
    """The relative bound on |got - ref| / S of the arithmetic that runs: K products summed in any order plus the
    epilogue's few additions in fp32; under x3 also the 2^-16 of each operand that hi + lo leaves out and the dropped
    lo.lo product."""
    b = (case.K + 16) * 2.0 ** -24
    return b + 3 * 2.0 ** -16 if case.route().x3 else b


def grid_units(case, inp):
    """max over outputs of sum_k |p||q| + epilogue magnitudes, in units of the data's grid (the largest power of two
    dividing every value): below 2^24 every partial sum, in any order, is an fp32 number."""
    P, Q = operands64(case, inp, True)
    _, S, _ = reference(case, inp, True)

    def unit(x):
        for e in range(4, -5, -1):
            if np.all(np.mod(x, 2.0 ** e) == 0):
                return 2.0 ** e
        raise AssertionError("data off every grid down to 2^-4")
    u = unit(P) * unit(Q)
    for k in ("bias", "addend", "C0"):
        if k in inp:
            u = min(u, unit(inp[k].astype(np.float64)))
    if "U" in inp:
        u = min(u, unit(inp["U"].astype(np.float64)) * unit(inp["V"].astype(np.float64)))
    return float(S.max()) / u
