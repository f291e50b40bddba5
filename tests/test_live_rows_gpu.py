"""The live-row count (include/wf3d.h "LIVE ROW COUNT"; set_edge_layout("padded", tail="skip")).

1. kernel contract, per entry point that honours a count: the row extent R spans several 256-row tiles; for live counts
   0, 1, 255, 256, 257, a mid value, R - 1 and R (a device tensor) the rows >= R256 of every row-indexed input hold NaN
   and those of every row-indexed output a sentinel; the rows < R256 and every reduced output are bit-equal to the same
   call without a count on inputs whose tail is zero, the sentinel rows are untouched, nothing is NaN.  The split GEMMs
   run under each forced kernel and automatically (one shape takes the persistent kernel, one splits K); the TN wgrad
   covers a zmap shape and a tn_rounds = 2 plan;
2. one captured call follows a new value of the same count tensor on replay;
3. EdgePredictor.forward_padded(tail="skip") equals tail="compute" bit for bit (probabilities, d vertices, all 24
   parameter gradients) at ragged counts with 0, 1 and V among them, at all counts < 2 and at all counts = V, in
   bf16x3 and bf16, eval and train; also on NaN-poisoned allocator memory; in fp32 it falls back and still equals;
4. skip mode at ragged counts against the fp64 oracle (method and bounds of tests/test_padded_edge_gpu.py part 3);
5. one captured train.py step with tail="skip", replayed over six batches, equals eager tail="compute" steps bit for bit.
"""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import helpers as H  # noqa: E402
from helpers import oracle  # noqa: E402
from oracle import dropout as D  # noqa: E402

SITE_PS = (0.05, 0.1, 0.2, 0.3)
SENT = 12345.0
NAN = float("nan")
GELU = 2


def dev():
    return torch.device("cuda:0")


@pytest.fixture
def device_rng():
    from wf3d import config
    old = config.dropout_rng()
    config.set_dropout_rng("device")
    try:
        yield
    finally:
        config.set_dropout_rng(old)


class _precision:
    def __init__(self, p):
        self.p = p

    def __enter__(self):
        from wf3d import config
        self.old = config.precision()
        config.set_precision(self.p)

    def __exit__(self, *exc):
        from wf3d import config
        config.set_precision(self.old)


# ---------------------------------------------------------------------------
# 1. kernel contract
# ---------------------------------------------------------------------------
def _r256(live, R):
    return min(R, -(-max(0, min(live, R)) // 256) * 256)


def _lives(R):
    return sorted({v for v in (0, 1, 255, 256, 257, (R // 2) | 1, R - 1, R) if 0 <= v <= R})


def _rand(*shape, seed=0, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dev())


def _sent(*shape):
    return torch.full(shape, SENT, dtype=torch.float32, device=dev())


def _tail(t, r, v):
    t = t.clone()
    t[r:] = v
    return t


def _contract(tag, R, inputs, rowin, fn, rowout, lives=None):
    """fn(inputs, count tensor | None) -> {name: output}; outputs named in `rowout` are row-indexed (dim 0), the others
    reduced.  Every output buffer is allocated by fn and pre-filled with SENT."""
    assert R >= 3 * 256, (tag, R)
    for live in (lives or _lives(R)):
        r = _r256(live, R)
        cnt = torch.tensor([live], dtype=torch.int32, device=dev())
        want = fn({k: _tail(t, r, 0.0) if k in rowin else t for k, t in inputs.items()}, None)
        got = fn({k: _tail(t, r, NAN) if k in rowin else t for k, t in inputs.items()}, cnt)
        torch.cuda.synchronize()
        assert set(got) == set(want)
        for k in got:
            g, w = got[k], want[k]
            if k in rowout:
                assert torch.equal(g[:r], w[:r]), (tag, live, k)
                assert bool((g[r:] == SENT).all()), (tag, live, k, "tail rows written")
                assert not bool(torch.isnan(g[:r]).any()), (tag, live, k)
            else:
                assert torch.equal(g, w), (tag, live, k)
                assert not bool(torch.isnan(g).any()), (tag, live, k)
                if live == 0 and not tag.endswith("+acc"):
                    assert not bool(g.any()), (tag, k, "reduced output of no rows is not zero")


def _gemm_split_fn(products, accumulate=False):
    from wf3d import ops

    def fn(inp, cnt):
        C = _sent(inp["A"].shape[0], inp["B"].shape[0])
        with ops.live_rows(cnt):
            ops.gemm_split(inp["A"], inp["B"], bias=inp.get("bias"), out=C, accumulate=accumulate, products=products)
        return {"C": C}
    return fn


# (M, N, K, accumulate): the persistent kernel's shape (512 full tiles, no split-K); a split-K shape (4 tiles of 256 rows,
# K cut 32 ways; under split_kernel 6 a partial 256-wide tile); 192 tiles with accumulate: the plain 256x256 kernel;
# a K that only the register-staged kernel takes (K % 32 != 0)
GEMM_SHAPES = [(32768, 1024, 256, False), (1024, 128, 4096, False), (1024, 128, 4096, True), (12288, 1024, 256, True),
               (1280, 200, 40, False)]


@pytest.mark.parametrize("kernel", [0, 1, 3, 6])
@pytest.mark.parametrize("shape", GEMM_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_contract_gemm_split(kernel, shape):
    from wf3d import _lib, ops
    M, N, K, acc = shape
    lib = _lib.load()
    if (M, N, K) == (32768, 1024, 256):
        assert lib.wf3d_gemm_split_ws_bytes(M, N, K) == 2048          # no split-K: the persistent kernel's control block
    if (M, N, K) == (1024, 128, 4096) and kernel in (0, 3):
        assert lib.wf3d_gemm_split_ws_bytes(M, N, K) == 32 * M * N * 4     # split-K, 32 ranges
    inputs = {"A": ops.split_rows(_rand(M, K, seed=1)), "B": ops.split_rows(_rand(N, K, seed=2)), "bias": _rand(N, seed=3)}
    with H.lib_option("split_kernel", kernel, default=0):
        for products in ((3, 1) if kernel == 0 else (3,)):
            lives = _lives(M) if M <= 2048 or products == 3 else [0, 257, M - 1]
            _contract(f"gemm_split k{kernel} p{products} {shape}" + ("+acc" if acc else ""), M, inputs, {"A"},
                      _gemm_split_fn(products, acc), {"C"}, lives)


def _gemm_tn_fn(products, accumulate=False):
    from wf3d import ops

    def fn(inp, cnt):
        C = _sent(inp["A"].shape[1], inp["B"].shape[1])
        with ops.live_rows(cnt):
            ops.gemm_split_tn(inp["A"], inp["B"], out=C, accumulate=accumulate, products=products)
        return {"C": C}
    return fn


# (Mo, No, K, tn_rounds, split_kernel): zmap (256x256 tiles, 56 ranges); the 256x128 kernel; the same shape forced onto it;
# a tn_rounds = 2 plan (16 tiles: 32 ranges instead of 16)
TN_SHAPES = [(256, 512, 16128, 1, 0), (256, 128, 16128, 1, 0), (256, 512, 16128, 1, 3), (256, 4096, 8192, 2, 0)]


@pytest.mark.parametrize("shape", TN_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_contract_gemm_split_tn(shape):
    from wf3d import _lib, ops
    Mo, No, K, rounds, kernel = shape
    lib = _lib.load()
    inputs = {"A": ops.split_rows(_rand(K, Mo, seed=4)), "B": ops.split_rows(_rand(K, No, seed=5))}
    with H.lib_option("tn_rounds", rounds, default=1), H.lib_option("split_kernel", kernel, default=0):
        ks = lib.wf3d_gemm_split_tn_ws_bytes(Mo, No, K) // (Mo * No * 4)
        if (Mo, No, K, kernel) == (256, 512, 16128, 0):
            assert ks == 56 and ks % 8 == 0                        # the zmap grid form
        if rounds == 2:
            assert ks == 32
            with H.lib_option("tn_rounds", 1, default=2):
                assert lib.wf3d_gemm_split_tn_ws_bytes(Mo, No, K) // (Mo * No * 4) == 16
        for products, acc in ((3, False), (1, False), (3, True)):
            _contract(f"gemm_split_tn p{products} {shape}" + ("+acc" if acc else ""), K, inputs, {"A", "B"},
                      _gemm_tn_fn(products, acc), set())


def test_contract_gemm_split_tn_single_range():
    """ksplit = 1 (an output of 256+ tiles would be too large here: a reduction too short to split): live = 0 must still
    leave exact zeros, or C itself under accumulate."""
    from wf3d import _lib, ops
    Mo, No, K = 256, 256, 224
    assert _lib.load().wf3d_gemm_split_tn_ws_bytes(Mo, No, K) == 0
    A, B = ops.split_rows(_rand(K, Mo, seed=4)), ops.split_rows(_rand(K, No, seed=5))
    want = _gemm_tn_fn(3)({"A": A, "B": B}, None)["C"]
    for live, ref in ((0, torch.zeros_like(want)), (1, want), (K, want)):
        cnt = torch.tensor([live], dtype=torch.int32, device=dev())
        got = _gemm_tn_fn(3)({"A": _tail(A, _r256(live, K), NAN), "B": _tail(B, _r256(live, K), NAN)}, cnt)["C"]
        assert torch.equal(got, ref), live
    cnt = torch.tensor([0], dtype=torch.int32, device=dev())
    got = _gemm_tn_fn(3, True)({"A": _tail(A, 0, NAN), "B": _tail(B, 0, NAN)}, cnt)["C"]
    assert bool((got == SENT).all())


def _ptrs():
    from wf3d import _lib, ops
    return _lib.load(), ops._p, ops._stream, _lib.check


@pytest.mark.parametrize("D,drop", [(256, 0.0), (512, 0.25), (384, 0.0)])
def test_contract_ln_prep(D, drop):
    from wf3d import ops
    lib, p, st, check = _ptrs()
    R = 1500
    inputs = {"z": _rand(R, D, seed=1), "gamma": _rand(D, seed=2), "beta": _rand(D, seed=3)}

    def fn(inp, cnt):
        mu, rs, h = _sent(R), _sent(R), _sent(R, D)
        with ops.live_rows(cnt):
            check(lib.wf3d_ln_prep(p(inp["z"]), R, D, p(inp["gamma"]), p(inp["beta"]), GELU, 1e-5, drop, 77, p(mu), p(rs), p(h),
                                   st()), "ln_prep")
        return {"mu": mu, "rs": rs, "h": h}
    _contract(f"ln_prep D={D}", R, inputs, {"z"}, fn, {"mu", "rs", "h"})


@pytest.mark.parametrize("D,drop,form", [(256, 0.3, "split"), (512, 0.0, "both"), (128, 0.0, "noln"), (2048, 0.0, "fp32")])
def test_contract_ln_act_bwd(D, drop, form):
    from wf3d import ops
    lib, p, st, check = _ptrs()
    R = 1100
    ln = form != "noln"
    inputs = {"dh": _rand(R, D, seed=1), "z": _rand(R, D, seed=2), "mu": _rand(R, seed=3, scale=0.1),
              "rs": _rand(R, seed=4).abs() + 0.5, "gamma": _rand(D, seed=5), "beta": _rand(D, seed=6)}

    def fn(inp, cnt):
        dz = _sent(R, D) if form in ("both", "fp32") else None
        dzs = _sent(R, D) if form != "fp32" else None
        trio = _sent(3, D)
        ws = ops.scratch(lib.wf3d_ln_act_bwd_ws_bytes(R, D), dev())
        with ops.live_rows(cnt):
            check(lib.wf3d_ln_act_bwd(p(inp["dh"]), p(inp["z"]), R, D, p(inp["mu"]) if ln else None, p(inp["rs"]) if ln else None,
                                      p(inp["gamma"]) if ln else None, p(inp["beta"]) if ln else None, GELU, drop, 5,
                                      p(dz), p(dzs), p(trio[0]), p(trio[1]), p(trio[2]), p(ws), ws.numel(), st()), "ln_act_bwd")
        out = {"trio": trio}
        if dz is not None:
            out["dz"] = dz
        if dzs is not None:
            out["dz_sx8"] = dzs
        return out
    _contract(f"ln_act_bwd D={D} {form}", R, inputs, {"dh", "z", "mu", "rs"}, fn, {"dz", "dz_sx8"})


@pytest.mark.parametrize("D", [512, 1536])
def test_contract_ln_act_bwd_wsum(D):
    from wf3d import ops
    lib, p, st, check = _ptrs()
    R = 1100
    inputs = {"dh": _rand(R, D, seed=1), "z": _rand(R, D, seed=2), "mu": _rand(R, seed=3, scale=0.1),
              "rs": _rand(R, seed=4).abs() + 0.5, "wrow": _rand(R, seed=7), "gamma": _rand(D, seed=5), "beta": _rand(D, seed=6)}

    def fn(inp, cnt):
        dz, duo, wsum = _sent(R, D), _sent(2, D), _sent(D)
        ws = ops.scratch(lib.wf3d_ln_act_bwd_wsum_ws_bytes(R, D), dev())
        with ops.live_rows(cnt):
            check(lib.wf3d_ln_act_bwd_wsum(p(inp["dh"]), p(inp["z"]), p(inp["wrow"]), R, D, p(inp["mu"]), p(inp["rs"]),
                                           p(inp["gamma"]), p(inp["beta"]), GELU, 0.2, 9, p(dz), None, p(duo[0]), p(duo[1]),
                                           p(wsum), p(ws), ws.numel(), st()), "ln_act_bwd_wsum")
        return {"dz": dz, "duo": duo, "wsum": wsum}
    _contract(f"ln_act_bwd_wsum D={D}", R, inputs, {"dh", "z", "mu", "rs", "wrow"}, fn, {"dz"})


def _pair_setup(counts, V, H_):
    from wf3d import ops
    B = len(counts)
    meta = ops.EdgeMeta.device(torch.tensor(counts, dtype=torch.int64, device=dev()), B, V)
    cv = _rand(meta.Rv, 3, seed=11)
    return meta, {"Pa": _rand(meta.Rv, H_, seed=12), "Pb": _rand(meta.Rv, H_, seed=13), "cv": cv, "wd": _rand(H_, seed=14),
                  "gamma": _rand(H_, seed=15), "beta": _rand(H_, seed=16)}


@pytest.mark.parametrize("H_,ln", [(512, True), (512, False), (256, True)])
@pytest.mark.parametrize("counts", [[24, 24, 24, 24], [24, 3, 0, 17]])
def test_contract_edge_pair_fwd(H_, ln, counts):
    """Both forms of pair_fwd.  With every count = V the layout has no tail of its own, so any live count applies."""
    from wf3d import ops
    lib, p, st, check = _ptrs()
    V = 24
    meta, inputs = _pair_setup(counts, V, H_)
    Re = meta.Re
    torch.cuda.synchronize()
    true_live = int(meta.eoff[-1])

    def fn(inp, cnt):
        pre, mu, rs, dl = _sent(Re, H_), _sent(Re), _sent(Re), _sent(Re)
        common = (p(inp["Pa"]), p(inp["Pb"]), p(inp["cv"]), p(inp["wd"]), 1, p(meta.voff), p(meta.eoff), p(meta.esample), Re, H_, 3,
                  1e-5, p(pre), p(mu), p(rs), p(dl))
        out = {"pre": pre, "mu": mu, "rs": rs, "delta": dl}
        with ops.live_rows(cnt):
            if ln:
                h = out["h"] = _sent(Re, H_)
                check(lib.wf3d_edge_pair_fwd_ln(*common, p(inp["gamma"]), p(inp["beta"]), GELU, 0.2, 3, p(h), st()), "pair_fwd_ln")
            else:
                check(lib.wf3d_edge_pair_fwd(*common, st()), "pair_fwd")
        return out
    lives = _lives(Re) if true_live == Re else [true_live]
    _contract(f"pair_fwd H={H_} ln={ln}", Re, inputs, set(), fn, {"pre", "mu", "rs", "delta", "h"}, lives)
    if true_live != Re:                      # the layout's own count: a view of eoff[B:], as EdgeFn passes it
        got = fn(inputs, meta.live)
        r = _r256(true_live, Re)
        for k, t in got.items():
            assert bool((t[r:] == SENT).all()) and not bool(t[true_live:r].any()), k


@pytest.mark.parametrize("H_", [512, 1024])
def test_contract_edge_pair_ln_bwd(H_):
    from wf3d import ops
    lib, p, st, check = _ptrs()
    V = 24
    meta, base = _pair_setup([V] * 4, V, H_)
    Re = meta.Re
    inputs = dict(base, dh=_rand(Re, H_, seed=1), delta=_rand(Re, seed=2).abs(), mu=_rand(Re, seed=3, scale=0.1),
                  rs=_rand(Re, seed=4).abs() + 0.5)

    def fn(inp, cnt):
        dz, duo, wsum = _sent(Re, H_), _sent(2, H_), _sent(H_)
        ws = ops.scratch(lib.wf3d_edge_pair_ln_bwd_ws_bytes(Re, H_), dev())
        with ops.live_rows(cnt):
            check(lib.wf3d_edge_pair_ln_bwd(p(inp["dh"]), p(inp["Pa"]), p(inp["Pb"]), p(inp["delta"]), p(inp["wd"]), 1, p(meta.voff),
                                            p(meta.eoff), p(meta.esample), Re, H_, p(inp["mu"]), p(inp["rs"]), p(inp["gamma"]),
                                            p(inp["beta"]), GELU, 0.2, 3, p(dz), p(duo[0]), p(duo[1]), p(wsum), p(ws), ws.numel(),
                                            st()), "edge_pair_ln_bwd")
        return {"dz": dz, "duo": duo, "wsum": wsum}
    _contract(f"edge_pair_ln_bwd H={H_}", Re, inputs, {"dh", "delta", "mu", "rs"}, fn, {"dz"})


@pytest.mark.parametrize("D", [128, 512, 8])
def test_contract_rowdot_act_and_bwd(D):
    from wf3d import ops
    lib, p, st, check = _ptrs()
    R = 1300
    inputs = {"z": _rand(R, D, seed=1), "t": _rand(R, seed=2), "w": _rand(D, seed=3), "bias": _rand(1, seed=4)}

    def fwd(inp, cnt):
        out = _sent(R, 1)
        with ops.live_rows(cnt):
            check(lib.wf3d_rowdot_act(p(inp["z"]), R, D, p(inp["w"]), p(inp["bias"]), GELU, p(out), st()), "rowdot_act")
        return {"out": out}

    def bwd(inp, cnt):
        dz, dzs, duo = _sent(R, D), _sent(R, D), _sent(2, D)
        ws = ops.scratch(lib.wf3d_rowdot_act_bwd_ws_bytes(R, D), dev())
        with ops.live_rows(cnt):
            check(lib.wf3d_rowdot_act_bwd(p(inp["z"]), p(inp["t"]), R, D, p(inp["w"]), GELU, p(dz), p(dzs), p(duo[0]), p(duo[1]),
                                          p(ws), ws.numel(), st()), "rowdot_act_bwd")
        return {"dz": dz, "dz_sx8": dzs, "duo": duo}
    _contract(f"rowdot_act D={D}", R, {k: inputs[k] for k in ("z", "w", "bias")}, {"z"}, fwd, {"out"})
    _contract(f"rowdot_act_bwd D={D}", R, inputs, {"z", "t"}, bwd, {"dz", "dz_sx8"})


@pytest.mark.parametrize("D,weighted", [(1, False), (128, True), (300, False)])
def test_contract_colsum(D, weighted):
    from wf3d import ops
    lib, p, st, check = _ptrs()
    R = 20000 if D == 1 else 1100                 # D = 1: the d logit column of a batch (2048 row blocks)
    inputs = {"x": _rand(R, D, seed=1)}
    if weighted:
        inputs["w"] = _rand(R, seed=2)

    def fn(inp, cnt):
        out = _sent(D)
        ws = ops.scratch(lib.wf3d_colsum_ws_bytes(R, D), dev())
        with ops.live_rows(cnt):
            check(lib.wf3d_colsum(p(inp["x"]), R, D, D, p(inp.get("w")), GELU if weighted else 0, p(out), p(ws), ws.numel(), st()),
                  "colsum")
        return {"out": out}
    _contract(f"colsum D={D}", R, inputs, {"x", "w"}, fn, set(), _lives(R) + [R + 1000])
    neg = fn(dict(inputs, x=_tail(inputs["x"], 0, NAN)), torch.tensor([-7], dtype=torch.int32, device=dev()))["out"]
    assert not bool(neg.any())                   # a negative count clamps to 0


@pytest.mark.parametrize("counts", [[24, 24, 24, 24], [24, 3, 0, 17]])
def test_contract_edge_prob_bwd(counts):
    from wf3d import ops
    lib, p, st, check = _ptrs()
    V = 24
    meta, _ = _pair_setup(counts, V, 8)
    Re, E = meta.Re, meta.max_e
    torch.cuda.synchronize()
    true_live = int(meta.eoff[-1])
    inputs = {"probs": torch.rand(len(counts), E, generator=torch.Generator().manual_seed(1)).to(dev()), "dprobs": _rand(len(counts), E, seed=2)}

    def fn(inp, cnt):
        dl = _sent(Re, 1)
        with ops.live_rows(cnt):
            check(lib.wf3d_edge_prob_bwd(p(inp["probs"]), p(inp["dprobs"]), p(meta.eoff), p(meta.esample), Re, E, p(dl), st()),
                  "edge_prob_bwd")
        return {"dlogit": dl}
    _contract("edge_prob_bwd", Re, inputs, set(), fn, {"dlogit"}, _lives(Re) if true_live == Re else [true_live])


@pytest.mark.parametrize("counts", [[24, 3, 0, 17], [1, 0, 1, 0]])
def test_pair_bwd_and_prob_fwd_never_read_the_tail(counts):
    """wf3d_edge_pair_bwd and wf3d_edge_prob_fwd take no count: they reach edge rows through eoff only.  NaN in every
    edge row past the live total of dpre / delta / logit changes nothing."""
    lib, p, st, check = _ptrs()
    V, H_ = 24, 512
    meta, inp = _pair_setup(counts, V, H_)
    Re, Rv, E, B = meta.Re, meta.Rv, meta.max_e, len(counts)
    torch.cuda.synchronize()
    live = int(meta.eoff[-1])
    assert live < Re - 256
    dpre, delta, logit = _rand(Re, H_, seed=1), _rand(Re, seed=2).abs() + 0.1, _rand(Re, 1, seed=3)
    wc = _rand(H_, 6, seed=4)

    def run(fill):
        dPa, dPb, dcv, probs = _sent(Rv, H_), _sent(Rv, H_), _sent(Rv, 3), _sent(B, E)
        check(lib.wf3d_edge_pair_bwd(p(_tail(dpre, live, fill)), p(_tail(delta, live, fill)), p(inp["cv"]), p(inp["wd"]), 1,
                                     p(meta.voff), p(meta.eoff), p(meta.vsample), Rv, H_, 3, p(dPa), p(dPb), p(dcv), p(wc), 6,
                                     st()), "edge_pair_bwd")
        check(lib.wf3d_edge_prob_fwd(p(_tail(logit, live, fill)), p(meta.eoff), B, E, p(probs), st()), "edge_prob_fwd")
        torch.cuda.synchronize()
        return dPa, dPb, dcv, probs
    for g, w in zip(run(NAN), run(0.0)):
        assert torch.equal(g, w) and not bool(torch.isnan(g).any()) and not bool((g == SENT).any())


@pytest.mark.parametrize("C,transpose", [(256, False), (64, False), (1104, True)])
def test_contract_split_rows(C, transpose):
    from wf3d import ops
    lib, p, st, check = _ptrs()
    R = 1104
    src = _rand(C, R, seed=1) if transpose else _rand(R, C, seed=1)       # transpose: out = split(src^T), rows = src's columns
    C_out = src.shape[0] if transpose else C

    def fn(inp, cnt):
        out = _sent(R, C_out)
        t = inp["t"]
        rs, cs = (1, t.stride(0)) if transpose else (t.stride(0), 1)
        with ops.live_rows(cnt):
            check(lib.wf3d_split_rows(p(t), rs, cs, R, C_out, p(out), st()), "split_rows")
        return {"out": out}
    if transpose:                           # the launch's rows are columns of the source: poison them there
        for live in _lives(R):
            r = _r256(live, R)
            cnt = torch.tensor([live], dtype=torch.int32, device=dev())
            z, n = src.clone(), src.clone()
            z[:, r:] = 0.0
            n[:, r:] = NAN
            want, got = fn({"t": z}, None)["out"], fn({"t": n}, cnt)["out"]
            torch.cuda.synchronize()
            assert torch.equal(got[:r], want[:r]) and bool((got[r:] == SENT).all()) and not bool(torch.isnan(got[:r]).any()), live
    else:
        _contract(f"split_rows C={C}", R, {"t": src}, {"t"}, fn, {"out"})


@pytest.mark.parametrize("form", ["sx8", "plain", "ln_drop"])
@pytest.mark.parametrize("C", [128, 200])
def test_contract_split_transpose(form, C):
    """The input's rows are the output's columns: under a count no input row >= R256 is read, the columns < R256 equal
    the call without a count and the columns [R256, R) are exact zeros (the reduction tail of the GEMM that follows)."""
    from wf3d import ops
    lib, p, st, check = _ptrs()
    R = 1104
    t = _rand(R, C, seed=1)
    if form == "sx8":
        t = ops.split_rows(t)
    mu, rs = _rand(R, seed=2, scale=0.1), _rand(R, seed=3).abs() + 0.5
    gamma, beta = _rand(C, seed=4), _rand(C, seed=5)
    ln = form == "ln_drop"

    def run(tt, m, r_, cnt):
        out = _sent(C, R)
        with ops.live_rows(cnt):
            check(lib.wf3d_split_transpose(p(tt), R, C, C, p(m) if ln else None, p(r_) if ln else None, p(gamma) if ln else None,
                                           p(beta) if ln else None, GELU if form != "sx8" else 0, 0.2 if ln else 0.0, 11,
                                           1 if form == "sx8" else 0, p(out), st()), "split_transpose")
        return out
    for live in _lives(R):
        r = _r256(live, R)
        cnt = torch.tensor([live], dtype=torch.int32, device=dev())
        want = run(_tail(t, r, 0.0), _tail(mu, r, 0.0), _tail(rs, r, 0.0), None)
        got = run(_tail(t, r, NAN), _tail(mu, r, NAN), _tail(rs, r, NAN), cnt)
        torch.cuda.synchronize()
        assert torch.equal(got[:, :r], want[:, :r]), (form, live)
        assert not bool(got[:, r:].any()) and not bool(torch.isnan(got).any()), (form, live)
        assert not bool((got == SENT).any()), (form, live)


def test_other_entry_points_ignore_the_count():
    """wf3d_gemm (the fp32 routes) and row_stats are documented as ignoring a count: with one set to 0 they still
    process every row."""
    from wf3d import ops
    a, b = _rand(600, 64, seed=1), _rand(48, 64, seed=2)
    want = (ops.gemm(a, b, ops.NT), ops.gemm(a, a, ops.TN), ops.row_stats(a))
    with ops.live_rows(torch.zeros(1, dtype=torch.int32, device=dev())):
        got = (ops.gemm(a, b, ops.NT), ops.gemm(a, a, ops.TN), ops.row_stats(a))
    torch.cuda.synchronize()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert torch.equal(got[2][0], want[2][0]) and torch.equal(got[2][1], want[2][1])
    assert bool(got[0][512:].any())


# ---------------------------------------------------------------------------
# 2. same pointer, new value
# ---------------------------------------------------------------------------
def _capture(fn):
    s = torch.cuda.Stream(dev())
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fn()
    return graph, out


def test_captured_call_follows_the_count_tensor():
    from wf3d import ops
    M, N, K = 1024, 128, 256
    A, B = ops.split_rows(_rand(M, K, seed=1)), ops.split_rows(_rand(N, K, seed=2))
    x = _rand(M, 64, seed=3)
    cnt = torch.tensor([300], dtype=torch.int32, device=dev())
    C = _sent(M, N)
    want_C = ops.gemm_split(A, B)

    def fn():
        with ops.live_rows(cnt):
            ops.gemm_split(A, B, out=C)
            return ops.colsum(x)
    graph, s = _capture(fn)
    for live in (300, 0, 700, 1024, 1):
        cnt.fill_(live)
        C.fill_(SENT)
        graph.replay()
        torch.cuda.synchronize()
        r = _r256(live, M)
        assert torch.equal(C[:r], want_C[:r]) and bool((C[r:] == SENT).all()), live
        assert torch.equal(s, ops.colsum(_tail(x, r, 0.0))), live
        assert (r == M) != (not torch.equal(s, ops.colsum(x))), live          # a shorter extent shows in the sum


# ---------------------------------------------------------------------------
# 3. model level: skip == compute, bit for bit
# ---------------------------------------------------------------------------
def _set_site_ps(ep, ps):
    ep.vertex_proj[5].p, ep.attention.dropout, ep.edge_mlp[3].p, ep.edge_mlp[7].p = ps
    return ep


def _run(ep, v, fn, cot):
    for p in ep.parameters():
        p.grad = None
    vg = v.clone().requires_grad_()
    out = fn(vg)
    (out * cot).sum().backward()
    return out.detach(), vg.grad, {n: p.grad for n, p in ep.named_parameters() if p.grad is not None}


class _live_spy:
    """Records what functional._edge_live decided, so that a silent fallback cannot pass for the skip path."""

    def __enter__(self):
        from wf3d import functional
        self.f, self.orig, self.seen, self.wgrads = functional, functional._edge_live, [], []

        def spy(meta, routes, fused_tail):
            out = self.orig(meta, routes, fused_tail)
            self.seen.append((meta.tail, out is not None, routes[0].fwd))
            self.wgrads.append(tuple(r.wgrad for r in routes))
            return out
        functional._edge_live = spy
        return self

    def __exit__(self, *exc):
        self.f._edge_live = self.orig


# 4 x 1128 = 4,512 edge rows: enough for the split route, and a multiple of 32, which the TN weight-gradient kernels need
# (multiples of 8 take the "transposes" wgrad: its own test below; other totals the fp32 wgrad, where skip computes the tail)
B3, V3 = 4, 48
COUNT_SETS = {"ragged": [48, 30, 1, 0], "none": [1, 0, 1, 0], "full": [48] * 4}


def _same(a, b):
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert len(a[2]) == 24 and set(a[2]) == set(b[2])
    for n in a[2]:
        assert bool(torch.isfinite(b[2][n]).all()), n
        assert torch.equal(a[2][n], b[2][n]), n


@pytest.mark.parametrize("precision", ["bf16x3", "bf16", "fp32"])
@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("which", list(COUNT_SETS))
def test_skip_equals_compute(precision, mode, which, device_rng):
    from models.EdgePredictor import EdgePredictor
    from wf3d import config
    from wf3d.random import default_generator
    assert B3 * V3 * (V3 - 1) // 2 >= config.SPLIT_MIN_ROWS
    torch.manual_seed(3)
    ep = _set_site_ps(EdgePredictor(3, 512, 8), SITE_PS).to(dev())
    ep.train() if mode == "train" else ep.eval()
    g = torch.Generator().manual_seed(8)
    v = torch.randn(B3, V3, 3, generator=g).to(dev())
    cot = torch.randn(B3, V3 * (V3 - 1) // 2, generator=g).to(dev())
    counts = torch.tensor(COUNT_SETS[which], dtype=torch.int64, device=dev())
    gen = default_generator(dev())
    with _precision(precision), _live_spy() as spy:
        st = gen.get_state()
        a = _run(ep, v, lambda x: ep.forward_padded(x, counts), cot)
        gen.set_state(st)
        b = _run(ep, v, lambda x: ep.forward_padded(x, counts, tail="skip"), cot)
    torch.cuda.synchronize()
    split = precision != "fp32"
    assert spy.seen == [("compute", False, "split" if split else "fp32"), ("skip", split, "split" if split else "fp32")], spy.seen
    _same(a, b)
    if split:
        assert set(spy.wgrads) == {("tn", "tn_t")}, spy.wgrads
    E = [c * (c - 1) // 2 for c in COUNT_SETS[which]]
    for s, e in enumerate(E):
        assert not bool(b[0][s, e:].any())
    if which == "none":
        assert not bool(b[0].any())


@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
@pytest.mark.parametrize("mode", ["eval", "train"])
def test_skip_equals_compute_on_the_transposes_route(precision, mode, device_rng):
    """5 x 1128 = 5,640 edge rows: a multiple of 8 but not of 32, so both wgrads take the "transposes" form
    (split_transpose + NT GEMM).  Skip mode runs under the count there too; also after a NaN fill of the allocator."""
    from models.EdgePredictor import EdgePredictor
    from wf3d.random import default_generator
    B, V, cl = 5, 48, [48, 30, 1, 0, 7]
    assert (B * V * (V - 1) // 2) % 8 == 0 and (B * V * (V - 1) // 2) % 32 != 0
    torch.manual_seed(3)
    ep = _set_site_ps(EdgePredictor(3, 512, 8), SITE_PS).to(dev())
    ep.train() if mode == "train" else ep.eval()
    g = torch.Generator().manual_seed(8)
    v = torch.randn(B, V, 3, generator=g).to(dev())
    cot = torch.randn(B, V * (V - 1) // 2, generator=g).to(dev())
    counts = torch.tensor(cl, dtype=torch.int64, device=dev())
    gen = default_generator(dev())
    with _precision(precision), _live_spy() as spy:
        st = gen.get_state()
        a = _run(ep, v, lambda x: ep.forward_padded(x, counts), cot)
        junk = torch.full((256 << 20,), NAN, dtype=torch.float32, device=dev())
        del junk
        gen.set_state(st)
        b = _run(ep, v, lambda x: ep.forward_padded(x, counts, tail="skip"), cot)
    torch.cuda.synchronize()
    assert spy.seen == [("compute", False, "split"), ("skip", True, "split")], spy.seen
    assert spy.wgrads == [("transposes", "transposes")] * 2, spy.wgrads
    _same(a, b)


@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
def test_skip_on_poisoned_memory(precision, device_rng):
    from models.EdgePredictor import EdgePredictor
    from wf3d.random import default_generator
    torch.manual_seed(9)
    ep = _set_site_ps(EdgePredictor(3, 512, 8), SITE_PS).to(dev()).train()
    g = torch.Generator().manual_seed(2)
    v = torch.randn(B3, V3, 3, generator=g).to(dev())
    cot = torch.randn(B3, V3 * (V3 - 1) // 2, generator=g).to(dev())
    counts = torch.tensor(COUNT_SETS["ragged"], device=dev())
    gen = default_generator(dev())
    st = gen.get_state()

    def run(fill, tail):
        junk = torch.full((256 << 20,), fill, dtype=torch.float32, device=dev())      # 1 GiB handed back to the cache
        del junk
        gen.set_state(st)
        return _run(ep, v, lambda x: ep.forward_padded(x, counts, tail=tail), cot)

    with _precision(precision), _live_spy() as spy:
        torch.cuda.synchronize()
        bad = run(NAN, "skip")
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        good = run(0.0, "compute")
        torch.cuda.synchronize()
    assert [s[:2] for s in spy.seen] == [("skip", True), ("compute", False)]
    assert bool(torch.isfinite(bad[0]).all()) and bool(torch.isfinite(bad[1]).all())
    _same(good, bad)


# ---------------------------------------------------------------------------
# 4. skip mode against the fp64 oracle
# ---------------------------------------------------------------------------
def test_skip_ragged_counts_vs_oracle(device_rng):
    """Method and bounds of tests/test_padded_edge_gpu.py part 3 (probabilities 1e-4, gradients 2e-4 in bf16x3)."""
    from models.EdgePredictor import EdgePredictor
    from wf3d import config
    counts, V, hidden, heads, ps = [40, 13, 1, 0], 48, 512, 8, SITE_PS
    assert len(counts) * V * (V - 1) // 2 >= config.SPLIT_MIN_ROWS and (len(counts) * V * (V - 1) // 2) % 32 == 0
    live = [c for c in counts if c >= 2]
    with _precision("bf16x3"), _live_spy() as spy:
        torch.manual_seed(5)
        ep = _set_site_ps(EdgePredictor(3, hidden, heads), ps).to(dev()).train()
        with torch.no_grad():
            for n, p_ in ep.named_parameters():
                if p_.dim() == 1:
                    p_.add_(0.05 * torch.randn(p_.shape, generator=torch.Generator().manual_seed(len(n))).to(dev()))
        g = torch.Generator().manual_seed(7)
        v = torch.randn(len(counts), V, 3, generator=g)
        vg = v.clone().to(dev()).requires_grad_()
        probs = ep.forward_padded(vg, torch.tensor(counts, device=dev()), tail="skip")
        words = [int(w) & 0xFFFFFFFF for w in ep.last_dropout_seeds.cpu().tolist()]
        cot = torch.randn(probs.shape, generator=g)
        (probs * cot.to(dev())).sum().backward()
        torch.cuda.synchronize()
    assert spy.seen == [("skip", True, "split")]
    masks = D.edge_head_masks(words[0], counts, ps, hidden, heads, s1=len(live))
    P = {"edge_predictor." + n: p_.detach().cpu().double().requires_grad_() for n, p_ in ep.named_parameters()}
    vr = v.double().requires_grad_()
    pc = probs.detach().cpu()
    errs, tot, e_out = {}, 0.0, 0.0
    for s, c in enumerate(counts):
        if c < 2:
            assert not pc[s].any(), s
            continue
        pr, _ = oracle.edge_forward(P, vr[s:s + 1, :c], num_heads=heads, drop=masks[s])
        E = pr.shape[1]
        e_out = max(e_out, H.elem_err(pc[s, :E].numpy(), pr[0].detach().numpy(), 1e-6))
        assert not pc[s, E:].any(), s
        tot = tot + (pr[0] * cot[s, :E].double()).sum()
    tot.backward()
    gv = vg.grad.cpu()
    for s, c in enumerate(counts):
        assert not gv[s, max(c, 0):].any(), s
    errs["<vertices>"] = H.elem_err(gv.numpy(), vr.grad.numpy())
    for n, p_ in ep.named_parameters():
        ref = P["edge_predictor." + n].grad
        if ref is None:
            assert p_.grad is None, n
            continue
        assert bool(torch.isfinite(p_.grad).all()), n
        errs[n] = H.elem_err(p_.grad.cpu().numpy(), ref.numpy())
    worst = sorted(((e, n) for n, e in errs.items()), reverse=True)
    print(f"skip, bf16x3, V={V}: probs {e_out:.2e} (bound 1e-4); worst gradient errors (bound 2e-4)",
          [(f"{e:.2e}", n) for e, n in worst[:4]])
    assert e_out < 1e-4, e_out
    bad = [(n, e) for n, e in errs.items() if not e < 2e-4]
    assert not bad, bad


# ---------------------------------------------------------------------------
# 5. one captured training step in skip mode
# ---------------------------------------------------------------------------
def _batches(n, B, N, V, seed):
    from wf3d.targets import train_targets
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        cnt = rng.integers(4, V + 1, size=B).tolist()
        vs = [rng.standard_normal((c, 3)).astype(np.float32) for c in cnt]
        es = [np.stack([np.arange(c - 1), np.arange(1, c)], 1) for c in cnt]
        t = train_targets(vs, es, V, device=dev(), full_width=True)
        t["x"] = torch.from_numpy(rng.standard_normal((B, N, 8)).astype(np.float32)).to(dev())
        out.append(t)
    assert len({tuple(b["vertex_counts"].tolist()) for b in out}) == n
    return out


def test_captured_skip_step_equals_eager_compute_steps(device_rng):
    from losses.WireframeLoss import WireframeLoss
    from models.PointCloudToWireframe import PointCloudToWireframe
    from wf3d import config
    from wf3d.meter import TrainMeter
    from wf3d.optim import ClipAdam
    from wf3d.random import default_generator
    B, N, V = 4, 2560, 32             # 4 x 496 = 1,984 edge rows: the split route with TN-kernel wgrads (a multiple of 32)
    assert B * V * (V - 1) // 2 >= config.SPLIT_MIN_ROWS and config.precision() in ("bf16x3", "bf16")
    torch.manual_seed(0)
    gen = default_generator(dev())
    model = PointCloudToWireframe(8, V).to(dev()).set_dropout(0.1).train().set_edge_layout("padded", tail="skip")
    twin = copy.deepcopy(model).set_edge_layout("padded", tail="compute")
    batches = _batches(7, B, N, V, seed=1)
    static = {k: t.clone() for k, t in batches[0].items()}
    crit = WireframeLoss(vertex_weight=3.0, edge_weight=1.0, existence_weight=1.5, assignment="device")

    def setup(m):
        opt = ClipAdam(m.parameters(), lr=1e-3, weight_decay=1e-6, max_norm=1.0, norm_params=m.parameters, capturable=True)
        return opt, TrainMeter(dev())

    def step(m, opt, meter, bt):
        opt.zero_grad()
        out = m(bt["x"], bt["vertex_counts"])
        res = crit(out, {k: bt[k] for k in ("vertices", "vertex_existence", "edge_labels", "vertex_counts")})
        res["total_loss"].backward()
        opt.step()
        meter.update(res, out["vertices"], bt["vertices"], bt["vertex_counts"])

    opt, meter = setup(model)
    opt2, meter2 = setup(twin)
    start = gen.get_state()
    torch.manual_seed(2)
    with _live_spy() as spy:
        graph, _ = _capture(lambda: step(model, opt, meter, static))
        assert spy.seen and all(s == ("skip", True, "split") for s in spy.seen), spy.seen
        gen.set_state(start)
        torch.manual_seed(2)
        n0 = len(spy.seen)
        for _ in range(2):
            step(twin, opt2, meter2, batches[0])
        assert all(s == ("compute", False, "split") for s in spy.seen[n0:]), spy.seen
    named2 = dict(twin.named_parameters())
    assert len(batches[1:]) >= 6
    for k, bt in enumerate(batches[1:]):
        for key, t in bt.items():
            static[key].copy_(t)
        before = gen.get_state()
        graph.replay()
        torch.cuda.synchronize()
        after = gen.get_state()
        gen.set_state(before)
        step(twin, opt2, meter2, bt)
        torch.cuda.synchronize()
        assert torch.equal(gen.get_state(), after)
        for n, p in model.named_parameters():
            assert torch.equal(p, named2[n]), (k, n)
            assert (p.grad is None) == (named2[n].grad is None) and (p.grad is None or torch.equal(p.grad, named2[n].grad)), (k, n)
    assert torch.equal(meter.state, meter2.state)
    hist = meter.read()["loss_history"]
    assert len(hist) == 2 + len(batches) - 1 and np.all(np.isfinite(hist))
