"""Every producer of the sx8 operand format, bit for bit against the integer model of tests/sx8_model.py.

The format (include/wf3d.h, csrc/split.hip): hi = bf16_rne(v), lo = bf16_rne(v - hi), 8 high parts then 8 low parts per
group of 8 columns.  Eleven entry points write it through four implementations of the split and of the lane-pair
exchange (store_sx8 in split.hip; wf3d_store_sx8_pair in wf3d_common.h; pair_store_sx8 in edge.hip; the dz_sx8 stores of
rowops.hip).  No assertion here has a tolerance: every one is equality of the raw container bits, of the bf16 bit
planes, or of fp32 bits.

The values are the payload of sx8_model.payload(): fp32 patterns on which every rounding of the split is live (ties in
hi onto either parity, carries into the next binade, low parts of the opposite sign, inexact low parts, ties of the low
part), laid over each matrix with a per-row rotation (sx8_model.tile) so that every class meets every column of a
group, both lanes of an exchanging pair and a row's first and last group.  Producers that compute a LayerNorm get the
payload through gamma: with eps = 0, beta = 0 and rows of +-a (a power of two, zero row sum) they must emit mu = 0,
rs = 1/a and h = act(+-gamma) exactly (tests/test_sx8_model.py shows why).  Producers that also have an fp32 form must
equal the model's split of that fp32 output.  Dropout forms use p = 0.5 (scale exactly 2) with the keep bits replayed by
oracle/dropout.py.  2^-60 <= |v| <= 2^60 throughout: bf16 subnormals, overflow and non-finite values are out of scope.

Code path per shape:

  split_rows          (37, 72) contiguous: vector loads; the same from a base 4 bytes off: scalar loads; transpose=True
                      and a row-strided view: the strided walk; (1, 8); (4100, 4096): 2 099 200 groups > 8192 * 256, the
                      grid-stride loop (model evaluated on the device).
  split_rows_multi    1, 2, 7, 8 jobs; W^T of (64, 128), (128, 192): the LDS 64 x 64 tile path; (72, 64), (64, 72), (8, 8),
                      (24, 40): the element path; a row-strided weight and one whose base is 4 bytes off; (1032, 4104):
                      529 416 groups per job > 2048 * 256 on the element path; (2112, 4096): 2112 tiles > 2048 on the tile
                      path (t += nblk); mixed sizes in one launch: blk_begin at every job boundary.
  split_transpose     (72, 36), (200, 1028), (136, 72): partial tiles in both directions; (64, 64), (128, 192): full tiles;
                      plain, identity prologue (act none / ReLU), in_sx8 (C % 8 == 0: the last three).
  ln_prep             D = 8, 136, 256: 32 lanes per row; 264 (NS 1), 512 (NS 1 FULL), 768 (NS 2), 1024 (NS 2 FULL), 1032
                      (NS 4), 2048 (NS 4 FULL), 4088 (NS 8), 4096 (NS 8 FULL); R = 1, 9 (one more than a multiple of the 8 or
                      4 rows of a workgroup), 13.
  first_layer         D = 8, 264, 512, 520, 1024 (NS 1 / 2); K = 8 aligned + ReLU + D % 512 == 0: FAST; K = 5, an x base 4
                      bytes off, or act none: not FAST; fwd (KEEP) and infer (!KEEP).
  edge pair           H = 64, 264 (NS 2, partial), 512, 1024 (NS 4); ragged counts with a sample of 2 vertices; a padded
                      device layout (zero tail rows); the block form at e0 = 8.
  pool4_bwd / seg     C = 8 (tpr 2), 24 (tpr 6: 256 % tpr != 0), 512 (tpr 128), 1024 (tpr 256), 2048 (two column blocks).
  ln_act_bwd_wsum     D = 8 (one wave per row) and 1032 (NS 2, four waves per row); rowdot_act_bwd: D = 8 and 512.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import helpers as H  # noqa: E402,F401  (sets sys.path)
import sx8_model as M  # noqa: E402
from oracle import dropout as D_  # noqa: E402

GUARD = 3                       # rows of guard band before and after an output
FILL = 0x5A5AC3C3               # their content: in no payload value and in no bf16 pair the model yields here
DROP_P, SEED = 0.5, 0x1234ABCD


@pytest.fixture(scope="module")
def ops():
    from wf3d import ops as o
    o._lib.load()
    return o


def dev():
    return torch.device("cuda:0")


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def bits(t):
    return t.contiguous().view(torch.int32)


def assert_sx8(tag, got, want_values):
    """`got` (sx8 device tensor [R, C]) holds exactly the model's container of the float32 array `want_values`."""
    want = to_dev(M.pack(np.asarray(want_values, dtype=np.float32)))
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    if not torch.equal(bits(got), bits(want)):
        (gh, gl), (wh, wl) = M.planes16(got), M.planes16(want)
        bad = ((gh != wh) | (gl != wl)).nonzero()
        r, c = (int(x) for x in bad[0])
        raise AssertionError(f"{tag}: {len(bad)} elements differ, first at ({r}, {c}): value {want_values[r][c]!r} "
                             f"hi {int(gh[r, c]) & 0xFFFF:#06x} / {int(wh[r, c]) & 0xFFFF:#06x} "
                             f"lo {int(gl[r, c]) & 0xFFFF:#06x} / {int(wl[r, c]) & 0xFFFF:#06x} (kernel / model)")


def assert_bits(tag, got, want):
    """fp32 tensors equal bit for bit (`want`: numpy or tensor)."""
    want = to_dev(np.asarray(want, dtype=np.float32)) if not torch.is_tensor(want) else want
    assert got.shape == want.shape and torch.equal(bits(got), bits(want)), tag


class Guarded:
    """A contiguous float32 [rows, cols] output placed inside a larger buffer of FILL words."""

    def __init__(self, rows, cols):
        self.buf = torch.full((rows + 2 * GUARD, cols), FILL, dtype=torch.int32, device=dev())
        self.view = self.buf[GUARD:GUARD + rows].view(torch.float32)
        assert self.view.data_ptr() % 16 == 0 and self.view.is_contiguous()
        self.rows = rows

    def check(self, tag):
        assert bool((self.buf[:GUARD] == FILL).all()) and bool((self.buf[GUARD + self.rows:] == FILL).all()), \
            f"{tag}: wrote outside its output"


def keep2(rows, cols, row0=0):
    """The factor of the dropout forms at p = 0.5: 2 where (row, col) is kept under SEED, else 0 (float32)."""
    assert D_.thresh_scale(DROP_P) == (1 << 31, np.float32(2))
    k = D_.keep(SEED, row0 + np.arange(rows)[:, None], np.arange(cols)[None, :], DROP_P)
    return np.where(k, np.float32(2), np.float32(0))


def dropped(v, k2):
    """keep ? 2 * v : +0 (never -0: the kernels write the literal 0.f)."""
    return np.where(k2 != 0, np.float32(2) * v, np.float32(0)).astype(np.float32)


def test_payload_holds_every_class():
    _, counts = M.payload()
    assert all(counts[k] > 0 for k in M.CLASSES), counts


# ---------------------------------------------------------------------------------------------------------------------
# split_rows
# ---------------------------------------------------------------------------------------------------------------------
def test_split_rows_forms(ops):
    R, C = 37, 72
    v = M.tile(R, C)
    assert_sx8("contiguous", ops.split_rows(to_dev(v)), v)
    flat = torch.zeros(R * C + 4, device=dev())
    off = flat[1:1 + R * C].view(R, C)
    off.copy_(to_dev(v))
    assert off.data_ptr() % 16 == 4
    assert_sx8("base 4 bytes off", ops.split_rows(off), v)
    wide = to_dev(M.tile(R, C + 12, off=5))
    assert_sx8("row-strided view", ops.split_rows(wide[:, 4:4 + C]), wide[:, 4:4 + C].cpu().numpy())
    vt = M.tile(C, R + 3, off=9)                                   # [72, 40] -> split of its transpose [40, 72]
    assert_sx8("transpose", ops.split_rows(to_dev(vt), transpose=True), vt.T)
    assert_sx8("transpose of a strided view", ops.split_rows(wide[:32, 4:44], transpose=True), wide[:32, 4:44].cpu().numpy().T)
    one = M.tile(1, 8, off=3)
    assert_sx8("1 x 8", ops.split_rows(to_dev(one)), one)


def tile_dev(R, C, off=0):
    p = to_dev(M.payload()[0])
    idx = (torch.arange(C, device=dev())[None, :] + M.ROT * torch.arange(R, device=dev())[:, None] + off) % p.numel()
    return p[idx]


def assert_planes_dev(tag, got, v):
    """The same assertion with the model evaluated in torch integer ops on the device (large matrices)."""
    hi, lo = M.split_torch(v)
    gh, gl = M.planes16(got)
    assert torch.equal(gh, M.bits16(hi)), f"{tag}: high plane"
    assert torch.equal(gl, M.bits16(lo)), f"{tag}: low plane"


def test_split_rows_past_the_block_cap(ops):
    R, C = 4100, 4096
    assert R * (C // 8) > 8192 * 256
    v = tile_dev(R, C)
    assert_planes_dev("split_rows grid-stride", ops.split_rows(v), v)


# ---------------------------------------------------------------------------------------------------------------------
# split_rows_multi (ops.split_weights)
# ---------------------------------------------------------------------------------------------------------------------
def multi(ops, jobs):
    """wf3d_split_rows_multi over jobs = [(src, row_stride, col_stride, R, C, out)]."""
    n = len(jobs)
    ins, outs = (ctypes.c_void_p * n)(), (ctypes.c_void_p * n)()
    rs, cs = (ctypes.c_long * n)(), (ctypes.c_long * n)()
    Rr, Cc = (ctypes.c_int * n)(), (ctypes.c_int * n)()
    for k, (src, r_, c_, R, C, out) in enumerate(jobs):
        assert tuple(out.shape) == (R, C) and out.is_contiguous()
        ins[k], outs[k], rs[k], cs[k], Rr[k], Cc[k] = src.data_ptr(), out.data_ptr(), r_, c_, R, C
    ops.check(ops._lib.load().wf3d_split_rows_multi(ins, rs, cs, Rr, Cc, outs, n, ops._stream()), "split_rows_multi")


def both(W, a=None, b=None):
    """The two jobs of a weight [N, K]: split(W) -> a [N, K], split(W^T) -> b [K, N]."""
    N, K = W.shape
    a = torch.empty(N, K, device=dev()) if a is None else a
    b = torch.empty(K, N, device=dev()) if b is None else b
    return [(W, W.stride(0), 1, N, K, a), (W, 1, W.stride(0), K, N, b)]


def small_weights():
    """Mixed sizes: tile path (both dims % 64 == 0) and element path, a row-strided view, a base 4 bytes off."""
    w = [to_dev(M.tile(n, k, off=o)) for n, k, o in ((64, 128, 0), (72, 64, 1), (8, 8, 2), (64, 72, 3))]
    strided = to_dev(M.tile(128, 200, off=4))[:, :192]                      # stride(0) = 200 > K = 192: tile path
    flat = torch.zeros(24 * 40 + 4, device=dev())
    off = flat[1:1 + 24 * 40].view(24, 40)
    off.copy_(to_dev(M.tile(24, 40, off=5)))
    assert off.data_ptr() % 16 == 4 and strided.stride(0) > strided.shape[1]
    return w + [strided, off]


def check_jobs(tag, jobs):
    for k, (src, r_, c_, R, C, out) in enumerate(jobs):
        W = src.cpu().numpy()
        assert_sx8(f"{tag} job {k}", out, W if c_ == 1 else W.T)


@pytest.mark.parametrize("njobs", [1, 2, 7, 8])
def test_split_rows_multi_job_counts(ops, njobs):
    ws = small_weights()
    order = {1: [5], 2: [0], 7: [4, 1, 0, 2], 8: [3, 5, 4, 2]}[njobs]
    jobs = sum((both(ws[i]) for i in order), [])[:njobs]
    # the last job writes into a guarded buffer
    src, r_, c_, R, C, _ = jobs[-1]
    g = Guarded(R, C)
    jobs[-1] = (src, r_, c_, R, C, g.view)
    multi(ops, jobs)
    check_jobs(f"{njobs} jobs", jobs)
    g.check(f"{njobs} jobs, last job")


def test_split_weights_wrapper(ops):
    ws = small_weights()
    for (a, b), W in zip(ops.split_weights(ws), ws):               # 6 weights: a launch of 8 jobs and one of 4
        assert_sx8("split_weights W", a, W.cpu().numpy())
        assert_sx8("split_weights W^T", b, W.cpu().numpy().T)


@pytest.mark.parametrize("N,K,what", [(1032, 4104, "element path past 2048 blocks"), (2112, 4096, "tile path past 2048 tiles")])
def test_split_rows_multi_past_the_block_caps(ops, N, K, what):
    assert N * (K // 8) > 2048 * 256 and ((N % 64 == 0 and K % 64 == 0 and (N // 64) * (K // 64) > 2048) or N % 64)
    W = tile_dev(N, K, off=7)
    small = to_dev(M.tile(8, 16, off=1))                           # a job boundary behind a capped job
    jobs = both(W) + both(small)
    multi(ops, jobs)
    assert_planes_dev(what + ", W", jobs[0][5], W)
    assert_planes_dev(what + ", W^T", jobs[1][5], W.T.contiguous())
    check_jobs(what, jobs[2:])


# ---------------------------------------------------------------------------------------------------------------------
# split_transpose
# ---------------------------------------------------------------------------------------------------------------------
def transpose_into(ops, t, out, pro=None, in_sx8=False):
    R, C = t.shape
    mu = rs = gamma = beta = None
    act, drop_p, seed = ops.ACT_NONE, 0.0, 0
    if pro is not None:
        mu, rs, gamma, beta, act, drop_p, seed = pro.mu, pro.rs, pro.gamma, pro.beta, pro.act, pro.drop_p, pro.seed
    p = ops._p
    ops.check(ops._lib.load().wf3d_split_transpose(p(t), R, C, t.stride(0), p(mu), p(rs), p(gamma), p(beta), act, float(drop_p),
                                                   int(seed) & 0xFFFFFFFF, 1 if in_sx8 else 0, p(out), ops._stream()), "split_transpose")


def identity_pro(ops, R, C, act, drop_p=0.0):
    one = lambda n: torch.ones(n, device=dev())                    # noqa: E731
    zero = lambda n: torch.zeros(n, device=dev())                  # noqa: E731
    return ops.Pro(act, zero(R), one(R), one(C), zero(C), drop_p, SEED)


@pytest.mark.parametrize("R,C", [(72, 36), (200, 1028), (136, 72), (64, 64), (128, 192)])
def test_split_transpose_forms(ops, R, C):
    v = M.tile(R, C, off=R)
    t = to_dev(v)
    for tag, pro, want in (("plain", None, v),
                           ("identity prologue", identity_pro(ops, R, C, ops.ACT_NONE), v),
                           ("identity prologue + ReLU", identity_pro(ops, R, C, ops.ACT_RELU), M.act_np(1, v))):
        g = Guarded(C, R)
        transpose_into(ops, t, g.view, pro)
        assert_sx8(f"split_transpose {tag}", g.view, want.T)
        g.check(f"split_transpose {tag}")
        assert torch.equal(bits(ops.split_transpose(t, pro)), bits(g.view))
    if C % 8 == 0:
        # in_sx8: the input's two planes, transposed — on planes that are the model's (among them low parts rounded up
        # onto half an ulp of an odd hi, which a second split of hi + lo would not return), and on a pair of planes that
        # is no value's split at all
        hi, lo = M.split(v)
        for tag, (ph, pl) in (("model planes", (hi, lo)), ("foreign planes", (hi, M.split(np.roll(v, 1, axis=1))[0]))):
            src = to_dev(M.pack_planes(ph, pl))
            g = Guarded(C, R)
            transpose_into(ops, src, g.view, in_sx8=True)
            want = to_dev(M.pack_planes(np.ascontiguousarray(ph.T), np.ascontiguousarray(pl.T)))
            assert torch.equal(bits(g.view), bits(want)), f"split_transpose in_sx8, {tag}"
            g.check(f"split_transpose in_sx8 {tag}")
            assert torch.equal(bits(ops.split_transpose(src, in_sx8=True)), bits(want))


def test_split_transpose_dropout(ops):
    R, C = 72, 36
    v = M.tile(R, C, off=2)
    out = ops.split_transpose(to_dev(v), identity_pro(ops, R, C, ops.ACT_RELU, DROP_P))
    assert_sx8("split_transpose dropout", out, dropped(M.act_np(1, v), keep2(R, C)).T)


# ---------------------------------------------------------------------------------------------------------------------
# ln_prep: the exact LayerNorm input, the payload in gamma
# ---------------------------------------------------------------------------------------------------------------------
A = 0.25


def ln_case(R, D, off):
    s = M.signs(R, D)
    gamma = M.tile(1, D, off=off)[0]
    return s, gamma, to_dev(s * np.float32(A)), to_dev(gamma), torch.zeros(D, device=dev())


def check_stats(tag, mu, rs, R, a=A):
    assert_bits(f"{tag} mu", mu, np.zeros(R, dtype=np.float32))
    assert_bits(f"{tag} rs", rs, np.full(R, 1.0 / a, dtype=np.float32))


@pytest.mark.parametrize("D", [8, 136, 256, 264, 512, 768, 1024, 1032, 2048, 4088, 4096])
def test_ln_prep_every_width(ops, D):
    # a width of 8 holds 8 payload values per call: walk the whole table; wider rows see it in one or two
    offs = range(0, M.payload()[0].size, 8) if D == 8 else (0, 601) if D < 1024 else (D,)
    for n, off in enumerate(offs):
        for R, act in ((9, n % 2), (1, 1 - n % 2), (13, 1 - n % 2)) if n < 2 else ((9, n % 2),):
            s, gamma, z, gd, bd = ln_case(R, D, off)
            want = M.act_np(act, s * gamma[None, :])
            tag = f"ln_prep D={D} R={R} act={act} off={off}"
            if R == 9:
                g, mu, rs = Guarded(R, D), torch.empty(R, device=dev()), torch.empty(R, device=dev())
                ops.ln_prep(z, gd, bd, act, eps=0.0, out=(mu, rs, g.view))
                h = g.view
                g.check(tag)
            else:
                mu, rs, h = ops.ln_prep(z, gd, bd, act, eps=0.0)
            check_stats(tag, mu, rs, R)
            assert_sx8(tag, h, want)


@pytest.mark.parametrize("D", [136, 1032])
def test_ln_prep_dropout(ops, D):
    R = 9
    s, gamma, z, gd, bd = ln_case(R, D, 17)
    mu, rs, h = ops.ln_prep(z, gd, bd, ops.ACT_RELU, eps=0.0, drop_p=DROP_P, seed=SEED)
    check_stats(f"ln_prep dropout D={D}", mu, rs, R)
    assert_sx8(f"ln_prep dropout D={D}", h, dropped(M.act_np(1, s * gamma[None, :]), keep2(R, D)))


# ---------------------------------------------------------------------------------------------------------------------
# first layer: x = +-e_k, W[:, k] = a * signs_k, bias = 0  ->  z = +-a * signs_k
# ---------------------------------------------------------------------------------------------------------------------
def first_case(R, K, D, off, x_off=False):
    S = M.signs(K, D)                                              # [K, D]: the sign row of input column k
    k = np.arange(R) % K
    xs = np.where((np.arange(R) // K) % 2 == 0, 1.0, -1.0).astype(np.float32)
    x = np.zeros((R, K), dtype=np.float32)
    x[np.arange(R), k] = xs
    s = xs[:, None] * S[k]                                         # [R, D]
    gamma = M.tile(1, D, off=off)[0]
    if x_off:
        flat = torch.zeros(R * K + 4, device=dev())
        xd = flat[1:1 + R * K].view(R, K)
        xd.copy_(to_dev(x))
        assert xd.data_ptr() % 16 == 4
    else:
        xd = to_dev(x)
    return s, gamma, xd, to_dev(np.ascontiguousarray(S.T) * np.float32(A)), to_dev(gamma)


@pytest.mark.parametrize("D", [8, 264, 512, 520, 1024])
@pytest.mark.parametrize("K,act,x_off", [(8, 1, False), (8, 0, False), (5, 1, False), (8, 1, True)])
def test_first_layer_fwd_and_infer(ops, D, K, act, x_off):
    R = 21
    offs = range(0, M.payload()[0].size, 56) if D == 8 else (D + K,)
    for off in offs:
        s, gamma, x, W, gd = first_case(R, K, D, off, x_off)
        zero = torch.zeros(D, device=dev())
        tag = f"first_layer D={D} K={K} act={act} x_off={x_off} off={off}"
        for bias in (zero, None):
            z, mu, rs, h = ops.first_layer_fwd(x, W, bias, gd, zero, act, eps=0.0)
            assert_bits(f"{tag} z", z, s * np.float32(A))
            check_stats(tag, mu, rs, R)
            assert_sx8(f"{tag} fwd", h, M.act_np(act, s * gamma[None, :]))
        g = Guarded(R, D)
        ops.first_layer_infer(x, W, zero, gd, zero, act, eps=0.0, out=g.view)
        assert torch.equal(bits(g.view), bits(h)), f"{tag}: infer != fwd"
        g.check(f"{tag} infer")


@pytest.mark.parametrize("D,K", [(512, 8), (264, 5)])
def test_first_layer_dropout(ops, D, K):
    R = 21
    s, gamma, x, W, gd = first_case(R, K, D, 29)
    zero = torch.zeros(D, device=dev())
    z, mu, rs, h = ops.first_layer_fwd(x, W, zero, gd, zero, ops.ACT_RELU, eps=0.0, drop_p=DROP_P, seed=SEED)
    assert_bits("first_layer dropout z", z, s * np.float32(A))
    check_stats("first_layer dropout", mu, rs, R)
    assert_sx8(f"first_layer dropout D={D}", h, dropped(M.act_np(1, s * gamma[None, :]), keep2(R, D)))


# ---------------------------------------------------------------------------------------------------------------------
# edge pair combine: coincident vertices (delta = 0), Pb = 0, Pa rows +-a  ->  pre[e] = Pa[i(e)]
# ---------------------------------------------------------------------------------------------------------------------
def pair_case(ops, counts, Hh, off, V=None):
    """V: a padded device layout of width V (tail rows belong to no sample)."""
    B = len(counts)
    if V is None:
        meta = ops.EdgeMeta(counts, dev())
        voff = np.concatenate([[0], np.cumsum(counts)])
    else:
        meta = ops.EdgeMeta.device(torch.tensor(counts, dtype=torch.int64, device=dev()), B, V)
        voff = np.concatenate([[0], np.cumsum(counts)])            # vertex rows are compact in both layouts
    first = [voff[b] + i for b, c in enumerate(counts) for i in range(c) for _ in range(i + 1, c)]
    S = M.signs(meta.Rv, Hh)
    s = S[np.array(first, dtype=np.int64)] if first else np.zeros((0, Hh), dtype=np.float32)
    gamma = M.tile(1, Hh, off=off)[0]
    g = torch.Generator().manual_seed(Hh)
    W0 = (0.2 * torch.randn(Hh, 2 * Hh + 7, generator=g)).to(dev())
    cv = torch.full((meta.Rv, 3), 0.375, device=dev())
    Pa, Pb = to_dev(S * np.float32(A)), torch.zeros(meta.Rv, Hh, device=dev())
    return meta, s, gamma, Pa, Pb, cv, W0, to_dev(gamma), torch.zeros(Hh, device=dev())


@pytest.mark.parametrize("Hh", [64, 264, 512, 1024])
@pytest.mark.parametrize("act", [0, 1])
def test_edge_pair_ln_output(ops, Hh, act):
    counts = [5, 2, 7, 3]
    offs = (0, 300, 600, 900) if Hh == 64 else (Hh + act,)
    for off in offs:
        meta, s, gamma, Pa, Pb, cv, W0, gd, bd = pair_case(ops, counts, Hh, off)
        Re = meta.Re
        assert s.shape == (Re, Hh)
        want = M.act_np(act, s * gamma[None, :])
        tag = f"edge_pair_fwd H={Hh} act={act} off={off}"
        pre, mu, rs, delta, h = ops.edge_pair_fwd(Pa, Pb, cv, W0, meta, eps=0.0, ln=(gd, bd, act, 0.0, 0))
        assert_bits(f"{tag} pre", pre, s * np.float32(A))
        assert_bits(f"{tag} delta", delta, np.zeros(Re, dtype=np.float32))
        check_stats(tag, mu, rs, Re)
        assert_sx8(tag, h, want)
        # the block form: rows [8, Re) into a guarded buffer
        g = Guarded(Re - 8, Hh)
        ops.edge_pair_infer(Pa, Pb, cv, W0, meta, 8, Re - 8, g.view, ln=(gd, bd, act), eps=0.0)
        assert torch.equal(bits(g.view), bits(h[8:])), f"{tag}: infer != fwd"
        g.check(f"{tag} infer")


def test_edge_pair_padded_layout_and_dropout(ops):
    Hh, V, counts = 264, 6, [4, 2, 6]
    meta, s, gamma, Pa, Pb, cv, W0, gd, bd = pair_case(ops, counts, Hh, 41, V=V)
    live = s.shape[0]
    assert meta.Re == 3 * 15 and live == 6 + 1 + 15
    Pa = torch.cat([Pa[:sum(counts)], torch.zeros(meta.Rv - sum(counts), Hh, device=dev())])
    Pb = torch.zeros(meta.Rv, Hh, device=dev())
    for p in (0.0, DROP_P):
        _, mu, rs, _, h = ops.edge_pair_fwd(Pa, Pb, cv, W0, meta, eps=0.0, ln=(gd, bd, ops.ACT_RELU, p, SEED))
        want = M.act_np(1, s * gamma[None, :])
        if p:
            want = dropped(want, keep2(live, Hh))
        assert_sx8(f"padded pair p={p}: live rows", h[:live], want)
        check_stats(f"padded pair p={p}", mu[:live], rs[:live], live)
        assert bool((bits(h[live:]) == 0).all()), "tail rows of a padded layout are all-zero bits"


# ---------------------------------------------------------------------------------------------------------------------
# producers with an fp32 form of the same value
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [8, 24, 512, 1024, 2048])
def test_pool4_bwd_sx8(ops, C):
    B, N = 3, 5
    g = torch.Generator().manual_seed(C)
    valid = (torch.rand(B * N, generator=g) > 0.3).float().to(dev())
    cnt = valid.view(B, N).sum(1).clamp(min=1)
    arg_m = torch.randint(0, N, (B, C), generator=g).int().to(dev())
    arg_u = torch.randint(0, N, (B, C), generator=g).int().to(dev())
    zero = torch.zeros(B, 2 * C, device=dev())
    rand = torch.randn(B, 2 * C, generator=g).to(dev())
    v = M.tile(B * N, C, off=C)
    direct = to_dev(v).view(B, N, C)
    lay = ops.PackedLayout.get([N] * B, dev())
    for tag, cot in (("payload", zero), ("random cotangents", rand)):
        cots = (cot[:, :C], cot[:, C:], cot[:, C:], cot[:, :C])
        args = (valid, cnt, arg_m, arg_u, *cots, direct)
        f32 = ops.pool4_bwd(*args, B, N, C).view(B * N, C)
        if cot is zero:
            assert_bits(f"pool4_bwd C={C}: 0 + 0 * valid + payload", f32, v)
        assert_sx8(f"pool4_bwd C={C} {tag}", ops.pool4_bwd(*args, B, N, C, sx8=True).view(B * N, C), f32.cpu().numpy())
        valid_pad = torch.zeros(lay.M_pad, device=dev())
        valid_pad[:B * N] = valid
        sargs = (valid_pad, cnt, arg_m, arg_u, *cots, direct.view(B * N, C))
        seg = ops.pool4_seg_bwd(*sargs, lay, C)
        s8 = ops.pool4_seg_bwd(*sargs, lay, C, sx8=True)
        assert seg.shape[0] == lay.M_pad and torch.equal(bits(seg[:B * N]), bits(f32))
        assert_sx8(f"pool4_seg_bwd C={C} {tag}", s8, seg.cpu().numpy())
        assert bool((bits(s8[B * N:]) == 0).all())


@pytest.mark.parametrize("C", [24, 1024])
def test_pool4_seg_bwd_sx8_ragged(ops, C):
    counts = [5, 1, 9]
    lay = ops.PackedLayout.get(counts, dev())
    Mr, B = lay.M, lay.B
    g = torch.Generator().manual_seed(C + 1)
    valid = torch.zeros(lay.M_pad, device=dev())
    valid[:Mr] = (torch.rand(Mr, generator=g) > 0.3).float().to(dev())
    cnt = torch.ones(B, device=dev())
    arg = torch.zeros(B, C, dtype=torch.int32, device=dev())
    zero = torch.zeros(B, 2 * C, device=dev())
    v = M.tile(Mr, C, off=3)
    args = (valid, cnt, arg, arg, zero[:, :C], zero[:, C:], zero[:, :C], zero[:, C:], to_dev(v))
    seg = ops.pool4_seg_bwd(*args, lay, C)
    assert_bits(f"pool4_seg_bwd C={C} fp32", seg[:Mr], v)
    s8 = ops.pool4_seg_bwd(*args, lay, C, sx8=True)
    assert_sx8(f"pool4_seg_bwd C={C} ragged", s8[:Mr], v)
    assert bool((bits(s8[Mr:]) == 0).all()) and bool((bits(seg[Mr:]) == 0).all())


@pytest.mark.parametrize("D", [8, 1032])
def test_ln_act_bwd_wsum_sx8(ops, D):
    R = 13
    g = torch.Generator().manual_seed(D)
    Z = (1.5 * torch.randn(R, D, generator=g) + 0.2).to(dev())
    gamma, beta = (1 + 0.2 * torch.randn(D, generator=g)).to(dev()), (0.1 * torch.randn(D, generator=g)).to(dev())
    # cotangent rows on scales 2^-20 .. 2^16, so that dz spans many binades
    dh = (torch.randn(R, D, generator=g) * torch.exp2(torch.arange(R) * 3.0 - 20)[:, None]).to(dev())
    wrow = torch.rand(R, generator=g).to(dev())
    mu, rs = ops.row_stats(Z)
    dz, duo, wsum = torch.empty_like(Z), torch.empty(2, D, device=dev()), torch.empty(D, device=dev())
    ds = Guarded(R, D)
    lib, p = ops._lib.load(), ops._p
    ws = ops.scratch(lib.wf3d_ln_act_bwd_wsum_ws_bytes(R, D), dev())
    ops.check(lib.wf3d_ln_act_bwd_wsum(p(dh), p(Z), p(wrow), R, D, p(mu), p(rs), p(gamma), p(beta), ops.ACT_RELU, 0.0, 0,
                                       p(dz), p(ds.view), p(duo[0]), p(duo[1]), p(wsum), p(ws), ws.numel(), ops._stream()),
              "ln_act_bwd_wsum")
    assert bool(torch.isfinite(dz).all()) and float(dz.abs().max()) > 0
    assert_sx8(f"ln_act_bwd_wsum D={D}", ds.view, dz.cpu().numpy())
    ds.check("ln_act_bwd_wsum")
    ds2 = torch.empty_like(Z)
    dz2, _, _, _ = ops.ln_act_bwd(dh, Z, mu, rs, gamma, beta, ops.ACT_RELU, dz_split=ds2)
    assert_sx8(f"ln_act_bwd D={D}", ds2, dz2.cpu().numpy())


@pytest.mark.parametrize("D", [8, 512])
def test_rowdot_act_bwd_sx8(ops, D):
    # dz[r, c] = t_r * w[c] * act'(z): with t = +-2^k and z > 0 under ReLU it is the payload in w, scaled exactly
    R = 21
    assert ops.rowdot_act_shape_ok(D)
    for off in (range(0, M.payload()[0].size, 56) if D == 8 else (5,)):
        w = M.tile(1, D, off=off)
        t = (np.where(np.arange(R) % 2 == 0, 1.0, -1.0) * np.exp2(np.arange(R) % 5 - 2)).astype(np.float32)
        z = torch.full((R, D), 0.5, device=dev())
        ds = Guarded(R, D)
        dz, _, _ = ops.rowdot_act_bwd(z, to_dev(t), to_dev(w), ops.ACT_RELU, dz_split=ds.view)
        assert_bits(f"rowdot_act_bwd D={D} dz", dz, t[:, None] * w)
        assert_sx8(f"rowdot_act_bwd D={D}", ds.view, dz.cpu().numpy())
        ds.check("rowdot_act_bwd")
