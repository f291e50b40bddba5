"""Route model, case table, data and fp64 reference of the split GEMM family (wf3d_gemm_split / wf3d_gemm_bf16 and their
_tn forms: csrc/gemm_split.hip, and the register-staged fallback wf3d_gemm_split_regs in csrc/gemm.hip).

TEST INFRASTRUCTURE ONLY, plain Python + numpy (no GPU, no library):

    route_nt / route_tn      the host decisions of gemm_split_impl / gemm_split_tn_impl restated from their code: kernel form,
                             tile grid, the split-K plan and what the workspace fit leaves of it, K slices per range, combine
                             kind, zmap, and every clause of persistent_ok by name.  tests/test_split_cases.py holds them to
                             the library's workspace queries and to its route query (wf3d_gemm_split_route / _tn_route), which
                             is the function the launch path itself decides with; DESIGN.md "wf3d_gemm_split: routes" is the
                             prose.
    CASES                    named cases, each the smallest shape that reaches one route or edge (`why`), with the route it
                             must reach (`form`, and where it matters ksplit / nks / combine / zmap / the persistent_ok
                             clauses that fail)
    inputs(case, data)       the operands as float32 arrays, data sets as gemm_cases.inputs defines them
    planes / reference       the sx8 planes (numpy, bit-exact RNE: tests/sx8_model.py) and, from them in float64, the result
                             each arithmetic defines: products = 3  sum_k ah.bh + ah.bl + al.bh;  products = 1  sum_k ah.bh;
                             plus bias and C0; and S, the same sum over absolute values

Operands as stored: NT  A = sx8[M, K], B = sx8[N, K];  TN  A = sx8[K, M], B = sx8[K, N]  (M = Mo, N = No).
"""
import dataclasses

import numpy as np

import gemm_cases as G
import sx8_model

cdiv = G.cdiv
SBK = 32
CTL_BYTES = 2048                   # the persistent kernel's control block
SCRATCH_MIN = 1 << 20              # wf3d.ops.scratch never hands out less
REGS, DMA3, X16, X16P, DMA3_TN, X16_TN = "regs", "dma3", "x16", "x16p", "dma3_tn", "x16_tn"
FORMS = (REGS, DMA3, X16, X16P, DMA3_TN, X16_TN)          # index = WF3D_SPLIT_FORM_*
COMBINES = ("none", "narrow", "wide")                     # index = WF3D_SPLIT_COMBINE_*
TILE = {REGS: (128, 128), DMA3: (256, 128), X16: (256, 256), X16P: (256, 256), DMA3_TN: (256, 128), X16_TN: (256, 256)}

# csrc/wf3d_common.h: nosplit_tiles, target, cap, few_tiles, few_slices, few_cap, few_mult8
RULE_GEMM = G.SPLITK_GEMM
RULE_SPLIT = (192, 512, 64, 0, 4, 64, False)
RULE_TN = (256, 512, 64, 4, 8, 256, True)
RULE_TN16 = (256, 256, 64, 4, 8, 256, True)


def splitk_plan(rule, tiles, ktotal, rounds=1):
    """(ksplit, kt_per) of wf3d_splitk_plan."""
    nosplit, target, cap, few_tiles, few_slices, few_cap, few_mult8 = rule
    if tiles >= nosplit or ktotal < 8:
        return 1, ktotal
    few = tiles <= few_tiles
    ks = min(cdiv(target * rounds, tiles), ktotal // (few_slices if few else 4), few_cap if few else cap * rounds)
    if few and few_mult8 and ks >= 8:
        ks &= ~7
    if ks < 2:
        return 1, ktotal
    kt_per = cdiv(ktotal, ks)
    return cdiv(ktotal, kt_per), kt_per


@dataclasses.dataclass(frozen=True)
class Opts:
    """The process-wide options that enter the route (wf3d_set_option)."""
    split_kernel: int = 0
    gemm_cus: int = 0
    tn_rounds: int = 1


@dataclasses.dataclass(frozen=True)
class Route:
    form: str
    nbm: int
    nbn: int
    ktotal: int
    planned: int          # K ranges the planner asks for (enters the workspace queries)
    ksplit: int           # after the workspace fit
    kt_per: int
    combine: str
    zmap: bool
    cus: int              # workgroups of the persistent kernel, else 0
    clauses: tuple        # ((name, holds), ...) of persistent_ok where it was asked, else ()

    @property
    def bm(self):
        return TILE[self.form][0]

    @property
    def bn(self):
        return TILE[self.form][1]

    @property
    def nks(self):
        return tuple(min(self.ktotal, (z + 1) * self.kt_per) - z * self.kt_per for z in range(self.ksplit))

    @property
    def failing(self):
        return tuple(n for n, ok in self.clauses if not ok)

    def as_query(self):
        """What wf3d_gemm_split_route / _tn_route write for this route."""
        return [FORMS.index(self.form), self.ksplit, self.kt_per, int(self.zmap), COMBINES.index(self.combine), self.nbm, self.nbn, self.cus]


def split_variant(M, N, kernel):
    if kernel in (3, 6):
        return kernel
    return 6 if cdiv(M, 256) * cdiv(N, 256) >= 192 and N % 256 == 0 else 3


def plan_regs(M, N, K):
    return splitk_plan(RULE_GEMM, cdiv(M, 128) * cdiv(N, 128), cdiv(K, SBK))


def plan_dma(M, N, K, variant):
    return splitk_plan(RULE_SPLIT, cdiv(M, 256) * cdiv(N, 256 if variant == 6 else 128), K // SBK)


def tn16(Mo, No, opts):
    return opts.split_kernel != 3 and Mo % 256 == 0 and No % 256 == 0


def plan_tn(Mo, No, K, opts):
    big = tn16(Mo, No, opts)
    tiles = cdiv(Mo, 256) * cdiv(No, 256 if big else 128)
    return splitk_plan(RULE_TN16 if big else RULE_TN, tiles, K // SBK, opts.tn_rounds if tiles >= 16 else 1)


def _slab(ks, M, N):
    return ks * M * N * 4 if ks > 1 else 0


def ws_bytes_nt(M, N, K, opts=Opts()):
    """wf3d_gemm_split_ws_bytes: room for the register-staged plan and the LDS-DMA one, at least the control block."""
    if min(M, N, K) <= 0:
        return 0
    ks = plan_dma(M, N, K, split_variant(M, N, opts.split_kernel))[0]
    return max(_slab(plan_regs(M, N, K)[0], M, N), _slab(ks, M, N) if ks > 1 else CTL_BYTES)


def ws_bytes_tn(Mo, No, K, opts=Opts()):
    return 0 if min(Mo, No, K) <= 0 else _slab(plan_tn(Mo, No, K, opts)[0], Mo, No)


def tn_ok(Mo, No, K, lda, ldb):
    return Mo > 0 and No > 0 and K >= SBK and Mo % 256 == 0 and No % 128 == 0 and K % SBK == 0 and lda % 4 == 0 and ldb % 4 == 0


def _fit(plan, ktotal, M, N, ws_addr, ws_bytes):
    need = _slab(plan[0], M, N)
    return (1, ktotal) if need and (ws_addr == 0 or ws_bytes < need) else plan


def _combine(form, ksplit, N, ws_addr):
    if ksplit == 1:
        return "none"
    return "wide" if form != REGS and ksplit > 16 and N % 4 == 0 and ws_addr % 16 == 0 else "narrow"


def persistent_clauses(M, N, K, lda, ldb, ldc, c_addr, bias_addr, accumulate, ksplit, ws_addr, ws_bytes, cus):
    """Every clause of persistent_ok, by name.  bias_addr None: no bias.  Addresses count modulo their alignment only."""
    tiles = cdiv(M, 256) * cdiv(N, 256)
    return (("one K range", ksplit == 1), ("no accumulate", not accumulate), ("M % 256", M % 256 == 0), ("N % 256", N % 256 == 0),
            (">= 8 slices", K // SBK >= 8), ("even slice count", K % (2 * SBK) == 0), ("workspace", ws_addr != 0),
            ("control block fits", ws_bytes >= CTL_BYTES), ("workspace % 64", ws_addr % 64 == 0), ("cus <= 384", cus <= 384),
            ("cus >= 8", cus >= 8), ("cus % 8", cus % 8 == 0), (">= 2 tiles per workgroup", tiles >= 2 * cus), ("ldc % 4", ldc % 4 == 0),
            ("lda rows fit 32 bits", lda * 1024 < 1 << 32), ("ldb rows fit 32 bits", ldb * 1024 < 1 << 32),
            ("ldc rows fit 32 bits", ldc * 1024 < 1 << 32), ("C % 16", c_addr % 16 == 0),
            ("bias % 16", bias_addr is None or bias_addr % 16 == 0))


def route_nt(M, N, K, lda, ldb, ldc, c_addr=0, bias_addr=None, accumulate=False, ws_addr=64, ws_bytes=1 << 40, cus=256, opts=Opts()):
    """gemm_split_impl.  ws_addr 0: no workspace.  cus: the device's compute units (gemm_cus is applied here)."""
    if opts.split_kernel == 1 or K % SBK:
        ktotal = cdiv(K, SBK)
        plan = plan_regs(M, N, K)
        ks, kt_per = _fit(plan, ktotal, M, N, ws_addr, ws_bytes)
        return Route(REGS, cdiv(M, 128), cdiv(N, 128), ktotal, plan[0], ks, kt_per, _combine(REGS, ks, N, ws_addr), False, 0, ())
    variant = split_variant(M, N, opts.split_kernel)
    ktotal = K // SBK
    plan = plan_dma(M, N, K, variant)
    ks, kt_per = _fit(plan, ktotal, M, N, ws_addr, ws_bytes)
    form, clauses, pc = (X16 if variant == 6 else DMA3), (), 0
    if variant == 6:
        if 8 <= opts.gemm_cus < cus:
            cus = opts.gemm_cus // 8 * 8
        clauses = persistent_clauses(M, N, K, lda, ldb, ldc, c_addr, bias_addr, accumulate, ks, ws_addr, ws_bytes, cus)
        if all(ok for _, ok in clauses):
            form, pc = X16P, cus
    return Route(form, cdiv(M, 256), cdiv(N, TILE[form][1]), ktotal, plan[0], ks, kt_per, _combine(form, ks, N, ws_addr), False, pc, clauses)


def route_tn(Mo, No, K, ws_addr=64, ws_bytes=1 << 40, opts=Opts()):
    """gemm_split_tn_impl (shapes that pass tn_ok)."""
    form = X16_TN if tn16(Mo, No, opts) else DMA3_TN
    ktotal = K // SBK
    plan = plan_tn(Mo, No, K, opts)
    ks, kt_per = _fit(plan, ktotal, Mo, No, ws_addr, ws_bytes)
    return Route(form, cdiv(Mo, 256), cdiv(No, TILE[form][1]), ktotal, plan[0], ks, kt_per, _combine(form, ks, No, ws_addr),
                 form == X16_TN and ks >= 8 and ks % 8 == 0, 0, ())


# ---- cases ---------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    why: str
    form: str                 # the kernel form the case is there for
    tn: bool
    M: int
    N: int
    K: int
    bias: bool = False
    accumulate: bool = False
    a_pad: int = 0            # extra columns of A's / B's / C's stored rows
    b_pad: int = 0
    ldc_pad: int = 0
    c_off: int = 0            # floats between a 16-B boundary and C's / the bias's first element
    bias_off: int = 0
    split_kernel: int = 0
    gemm_cus: int = 0
    tn_rounds: int = 1
    ws: object = None         # None: what the library's query asks for; "null"; or a byte count
    nks: tuple = None         # expected K slices per range, where the case is there for them
    combine: str = None       # expected combine kind
    zmap: bool = None
    fails: tuple = None       # the persistent_ok clauses that must be the only false ones (fallback cases)

    @property
    def opts(self):
        return Opts(self.split_kernel, self.gemm_cus, self.tn_rounds)

    @property
    def lda(self):
        return (self.M if self.tn else self.K) + self.a_pad

    @property
    def ldb(self):
        return (self.N if self.tn else self.K) + self.b_pad

    @property
    def ldc(self):
        return self.N + self.ldc_pad

    def ws_query(self):
        return ws_bytes_tn(self.M, self.N, self.K, self.opts) if self.tn else ws_bytes_nt(self.M, self.N, self.K, self.opts)

    def ws_given(self, mode):
        """(address, bytes) class of the workspace under a mode of gemm_gpu_util.workspace, as wf3d.ops passes it."""
        ask = self.ws_query()
        if isinstance(mode, int):
            return 64, mode
        if mode == "null" or ask <= 0:
            return 0, 0
        return 64, (max(ask, SCRATCH_MIN) if mode is None else ask - 1)

    def route_at(self, ws_addr, ws_bytes, c_addr=None, bias_addr=None, cus=256):
        if self.tn:
            return route_tn(self.M, self.N, self.K, ws_addr, ws_bytes, self.opts)
        c_addr = 4 * self.c_off if c_addr is None else c_addr
        bias_addr = (4 * self.bias_off if bias_addr is None else bias_addr) if self.bias else None
        return route_nt(self.M, self.N, self.K, self.lda, self.ldb, self.ldc, c_addr, bias_addr, self.accumulate, ws_addr, ws_bytes,
                        cus, self.opts)

    def route(self, ws="case", cus=256):
        return self.route_at(*self.ws_given(self.ws if ws == "case" else ws), cus=cus)


CASES = []
P_OPTS = dict(split_kernel=6, gemm_cus=8, ws=CTL_BYTES)       # the persistent kernel at 16+ tiles: see _build


def _nt(name, why, form, M, N, K, **kw):
    CASES.append(Case(name, why, form, False, M, N, K, **kw))


def _tn(name, why, form, M, N, K, **kw):
    CASES.append(Case(name, why, form, True, M, N, K, **kw))


def _build():
    # -- regs: K % 32 != 0, or split_kernel 1; 128x128 tiles; its combine is always the narrow one
    _nt("regs_k8", "K = 8: one partial slice", REGS, 100, 60, 8, nks=(1,))
    _nt("regs_k40", "K = 40, partial 128x128 tiles, N % 4 != 0", REGS, 130, 130, 40, bias=True, nks=(2,))
    _nt("regs_k104", "K = 104, padded rows", REGS, 200, 132, 104, bias=True, accumulate=True, a_pad=8, b_pad=16, ldc_pad=3, nks=(4,))
    _nt("regs_forced", "K % 32 == 0 under split_kernel 1", REGS, 256, 256, 96, split_kernel=1, bias=True, nks=(3,))
    _nt("regs_odd_N", "partial tiles, N % 4 != 0 with a gap", REGS, 129, 127, 40, ldc_pad=2)
    _nt("regs_split2", "two K ranges, the last slice partial", REGS, 100, 60, 232, bias=True, nks=(4, 4), combine="narrow")
    _nt("regs_split_uneven", "two K ranges, the last one shorter", REGS, 100, 61, 264, bias=True, accumulate=True, nks=(5, 4),
        combine="narrow")
    _nt("regs_split18", "18 ranges with N % 4 == 0: still the narrow combine", REGS, 64, 64, 2280, nks=(4,) * 18, combine="narrow")
    _nt("regs_forced_split", "split_kernel 1 on a 32-divisible K that splits", REGS, 128, 128, 256, split_kernel=1, accumulate=True,
        nks=(4, 4))

    # -- dma3: 256x128 tiles, three LDS stages
    _nt("dma3_nk1", "one slice: the prologue alone", DMA3, 256, 128, 32, nks=(1,))
    _nt("dma3_nk2", "two slices; partial tiles both ways, N % 4 != 0", DMA3, 300, 130, 64, bias=True, nks=(2,))
    _nt("dma3_nk3", "three slices: the first `ahead`", DMA3, 256, 128, 96, accumulate=True, ldc_pad=5, nks=(3,))
    _nt("dma3_nk4", "four slices: the stage ring wraps", DMA3, 512, 256, 128, a_pad=8, b_pad=24, nks=(4,))
    _nt("dma3_M300", "M % 256 != 0", DMA3, 300, 128, 64)
    _nt("dma3_N200", "N % 128 != 0", DMA3, 256, 200, 64, bias=True)
    _nt("dma3_N130", "N % 4 != 0 with a gap behind it", DMA3, 256, 130, 64, ldc_pad=2)
    _nt("dma3_9tiles", "9 tiles: not a multiple of the 8 XCDs", DMA3, 768, 384, 64)
    _nt("dma3_bias_acc", "bias and accumulate in the kernel", DMA3, 256, 128, 96, bias=True, accumulate=True)
    _nt("dma3_split2", "two K ranges, bias through the combine", DMA3, 256, 128, 256, bias=True, nks=(4, 4), combine="narrow")
    _nt("dma3_split9", "9 slices: ranges of 5 and 4; partial tiles", DMA3, 300, 130, 288, accumulate=True, nks=(5, 4), combine="narrow")
    _nt("dma3_split17_wide", "17 ranges, N % 4 == 0: wide combine, bias and accumulate", DMA3, 100, 128, 2176, bias=True,
        accumulate=True, ldc_pad=4, nks=(4,) * 17, combine="wide")
    _nt("dma3_split17_narrow", "17 ranges, N % 4 != 0: narrow combine", DMA3, 100, 126, 2176, bias=True, nks=(4,) * 17, combine="narrow")
    _nt("dma3_forced", "split_kernel 3 on a 256-divisible output", DMA3, 512, 512, 64, split_kernel=3)

    # -- x16: split_kernel 6 runs the plain 256x256 kernel on any shape
    _nt("x16_nk1", "256 x 256 x 32: one slice (odd count: the tail)", X16, 256, 256, 32, split_kernel=6, nks=(1,))
    _nt("x16_nk2", "two slices", X16, 256, 256, 64, split_kernel=6, bias=True, nks=(2,))
    _nt("x16_nk3", "three slices", X16, 256, 256, 96, split_kernel=6, accumulate=True, nks=(3,))
    _nt("x16_partial", "partial tiles both ways", X16, 300, 300, 64, split_kernel=6, bias=True, a_pad=8, b_pad=8, ldc_pad=4)
    _nt("x16_N258", "N % 4 != 0: the last column group is scalar", X16, 260, 258, 64, split_kernel=6, bias=True, ldc_pad=2)
    _nt("x16_5tiles", "5 tiles over 8 XCDs", X16, 1280, 256, 64, split_kernel=6)
    _nt("x16_c_off", "C one float past a 16-byte boundary: scalar stores", X16, 256, 256, 64, split_kernel=6, bias=True, accumulate=True,
        c_off=1, ldc_pad=4)
    _nt("x16_ldc_odd", "ldc % 4 != 0: scalar stores", X16, 256, 256, 64, split_kernel=6, bias=True, ldc_pad=2)
    _nt("x16_split_acc", "two K ranges, bias and accumulate through the combine", X16, 256, 256, 256, split_kernel=6, bias=True,
        accumulate=True, nks=(4, 4), combine="narrow")
    _nt("x16_split_N258", "two K ranges into slabs with N % 4 != 0", X16, 256, 258, 288, split_kernel=6, nks=(5, 4), combine="narrow")
    _nt("x16_split17", "17 ranges: wide combine", X16, 256, 256, 2176, split_kernel=6, bias=True, nks=(4,) * 17, combine="wide")

    # -- x16p: under 192 tiles the planner splits K whenever there are the 8 slices the persistent kernel needs, so the
    # persistent kernel is reached at 16 tiles through a workspace that holds its control block and no slab
    _nt("x16p_k256", "16 tiles on 8 workgroups, 8 slices (the minimum)", X16P, 1024, 1024, 256, **P_OPTS)
    _nt("x16p_k320", "10 slices, accumulators from zero: the bits of the plain kernel on any data", X16P, 1024, 1024, 320, **P_OPTS)
    _nt("x16p_k320_bias", "10 slices, bias as the accumulators' initial value", X16P, 1024, 1024, 320, bias=True, **P_OPTS)
    _nt("x16p_20tiles", "20 tiles: 4 XCD labels own 3, the others 2", X16P, 1280, 1024, 256, bias=True, **P_OPTS)
    _nt("x16p_nbn1", "one tile column (4608 x 256)", X16P, 4608, 256, 256, bias=True, **P_OPTS)
    _nt("x16p_cus16", "gemm_cus 16: two workgroups per label draw 32 tiles", X16P, 2048, 1024, 256, bias=True,
        **dict(P_OPTS, gemm_cus=16))
    _nt("x16p_padded", "lda, ldb, ldc padded", X16P, 1024, 1024, 256, bias=True, a_pad=8, b_pad=24, ldc_pad=4, **P_OPTS)

    # -- persistent fallbacks: x16p_k256 (+ bias) with one clause of persistent_ok falsified at a time
    base = dict(P_OPTS, bias=True)
    fb = lambda name, why, M=1024, N=1024, K=256, **kw: _nt("x16_fb_" + name, "persistent_ok fails on: " + why, X16, M, N, K,  # noqa: E731
                                                             **dict(base, **kw))
    fb("accumulate", "accumulate", accumulate=True, fails=("no accumulate",))
    fb("6slices", "fewer than 8 slices (an even count)", K=192, fails=(">= 8 slices",))
    fb("7slices", "7 slices: too few and odd", K=224, fails=(">= 8 slices", "even slice count"))
    fb("9slices", "an odd slice count (K = 288)", K=288, fails=("even slice count",))
    fb("M1000", "M % 256 != 0", M=1000, fails=("M % 256",))
    fb("N1000", "N % 256 != 0", N=1000, fails=("N % 256",))
    fb("ldc", "ldc % 4 != 0", ldc_pad=2, fails=("ldc % 4",))
    fb("c_off", "C one float past a 16-byte boundary", c_off=1, ldc_pad=4, fails=("C % 16",))
    fb("bias_off", "bias one float past a 16-byte boundary", bias_off=1, fails=("bias % 16",))
    fb("no_ws", "no workspace", ws="null", fails=("workspace", "control block fits"))
    fb("short_ws", "a workspace one byte short of the control block", ws=CTL_BYTES - 1, fails=("control block fits",))
    fb("15tiles", "fewer than 2 x cus tiles", M=768, N=1280, fails=(">= 2 tiles per workgroup",))
    fb("split", "room for the slabs: K is split", ws=None, fails=("one K range",), nks=(4, 4), combine="narrow")

    # -- dma3_tn: wgrad on 256x128 tiles (No % 256 != 0, or split_kernel 3)
    _tn("tn3_nk1", "one slice", DMA3_TN, 256, 128, 32, nks=(1,))
    _tn("tn3_nk2", "two slices, accumulate into a strided C", DMA3_TN, 256, 128, 64, accumulate=True, ldc_pad=3, nks=(2,))
    _tn("tn3_nk3", "three slices; padded operand rows", DMA3_TN, 256, 128, 96, a_pad=4, b_pad=8, nks=(3,))
    _tn("tn3_No384", "No % 256 != 0: 6 tiles", DMA3_TN, 512, 384, 128, nks=(4,))
    _tn("tn3_forced", "split_kernel 3 on a 256-divisible output", DMA3_TN, 256, 256, 64, split_kernel=3)
    _tn("tn3_split2", "two K ranges (no zmap on this kernel)", DMA3_TN, 256, 128, 512, accumulate=True, nks=(8, 8), combine="narrow",
        zmap=False)
    _tn("tn3_split_uneven", "17 slices: ranges of 9 and 8", DMA3_TN, 256, 128, 544, nks=(9, 8), combine="narrow")
    _tn("tn3_split32", "32 K ranges: wide combine into a strided C", DMA3_TN, 256, 128, 8192, ldc_pad=4, nks=(8,) * 32, combine="wide",
        zmap=False)

    # -- x16_tn: wgrad on 256x256 tiles
    _tn("tn16_nk1", "one slice", X16_TN, 256, 256, 32, nks=(1,))
    _tn("tn16_nk2", "two slices", X16_TN, 256, 256, 64, accumulate=True, nks=(2,))
    _tn("tn16_nk3", "three slices; ldc > No, lda > Mo", X16_TN, 256, 256, 96, a_pad=4, b_pad=12, ldc_pad=5, nks=(3,))
    _tn("tn16_4tiles", "4 tiles, 7 slices: no split", X16_TN, 512, 512, 224, nks=(7,))
    _tn("tn16_split2", "2 K ranges: the 3-D grid (no zmap)", X16_TN, 256, 256, 512, nks=(8, 8), combine="narrow", zmap=False)
    _tn("tn16_split8", "8 K ranges: the XCD-mapped 1-D grid", X16_TN, 256, 256, 2048, accumulate=True, nks=(8,) * 8, combine="narrow",
        zmap=True)
    _tn("tn16_65slices", "65 slices: 8 ranges, the last one of 2", X16_TN, 256, 256, 2080, nks=(9,) * 7 + (2,), zmap=True)
    _tn("tn16_split16_2tiles", "16 ranges x 2 tiles under zmap; ldc > No, lda > Mo", X16_TN, 256, 512, 4096, a_pad=4, b_pad=4,
        ldc_pad=4, nks=(8,) * 16, zmap=True)
    _tn("tn16_16tiles", "16 tiles x 16 ranges under zmap", X16_TN, 1024, 1024, 2048, nks=(4,) * 16, combine="narrow", zmap=True)
    _tn("tn16_rounds2", "tn_rounds 2 on 16 tiles: 17 ranges instead of 14, wide combine", X16_TN, 1024, 1024, 2176, tn_rounds=2,
        nks=(4,) * 17, combine="wide", zmap=False)


_build()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES), "duplicate case names"
PRODUCTS = (3, 1)


# ---- data and reference ----------------------------------------------------------------------------------------------
def as_gemm_case(case):
    """The gemm_cases.Case with this case's layout, shape and epilogue terms: what gemm_cases.inputs draws from."""
    return G.Case(case.name, case.why, G.TN if case.tn else G.NT, case.M, case.N, case.K, bias=case.bias, accumulate=case.accumulate)


def inputs(case, data):
    """{"A", "B" as stored (float32), "bias" [N], "C0" [M, N]}: gemm_cases.inputs on the same shape."""
    return G.inputs(as_gemm_case(case), data)


def exact_sets(products):
    return G.DATA_EXACT if products == 3 else ("int",)


def planes(case, inp):
    """(ph, pl, qh, ql) in float64 in the product's orientation, P [M, K] and Q [K, N], from the sx8 split of the operands."""
    (ah, al), (bh, bl) = sx8_model.split(inp["A"]), sx8_model.split(inp["B"])
    f = lambda x, t: (x.T if t else x).astype(np.float64)        # noqa: E731
    return f(ah, case.tn), f(al, case.tn), f(bh, not case.tn), f(bl, not case.tn)


def packed(inp):
    """The sx8 containers of A and B (float32 arrays of the operands' own shapes)."""
    return sx8_model.pack(inp["A"]), sx8_model.pack(inp["B"])


X3 = {"hh": 1, "hl": 1, "lh": 1, "ll": 0}       # weights of the plane products ah.bh, ah.bl, al.bh, al.bl under products = 3
X1 = {"hh": 1, "hl": 0, "lh": 0, "ll": 0}


def plane_products(case, inp, keys=("hh", "hl", "lh", "ll"), matmul=np.matmul, absolute=False):
    """{"hh": sum_k ah.bh, "hl": sum_k ah.bl, "lh": sum_k al.bh, "ll": sum_k al.bl} [M, N] in float64 (absolute: of |.|)."""
    ph, pl, qh, ql = (np.abs(x) if absolute else x for x in planes(case, inp))
    P, Q = {"h": ph, "l": pl}, {"h": qh, "l": ql}
    return {k: (matmul(P[k[0]], Q[k[1]]) if P[k[0]].any() and Q[k[1]].any() else np.zeros((case.M, case.N))) for k in keys}


def reference(case, inp, products, weights=None, matmul=np.matmul):
    """(ref, S) in float64 from the planes: ref = sum_k of the weighted plane products (default: what `products` defines)
    + bias + C0, S the same over absolute values.  matmul: any float64 product of two arrays (the GPU test brings its own)."""
    w = weights or (X3 if products == 3 else X1)
    keys = [k for k in w if w[k]]
    pp, pa = plane_products(case, inp, keys, matmul), plane_products(case, inp, keys, matmul, absolute=True)
    ref, S = sum(w[k] * pp[k] for k in keys), sum(abs(w[k]) * pa[k] for k in keys)
    for k, f in (("bias", lambda t: t[None, :]), ("C0", lambda t: t)):
        if k in inp:
            t = f(inp[k].astype(np.float64))
            ref, S = ref + t, S + np.abs(t)
    return ref, S


def bound(case):
    """|got - ref| <= bound * S_ij: K products summed in any order plus the epilogue's and the combine's few additions, in
    fp32 (DESIGN.md "wf3d_gemm_split: routes").  No splitting term: the reference is taken from the planes."""
    return (case.K + 16) * 2.0 ** -24
