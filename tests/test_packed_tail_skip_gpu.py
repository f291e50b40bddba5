"""Packed capacity batches with tail="skip": the encoder stops at the live row total (include/wf3d.h "LIVE ROW COUNT";
set_packed_tail("skip") of PointNetEncoder / PointCloudToWireframe, then encode_packed / forward_packed(..., capacity=)).
In the docstrings below tail="skip" / tail="compute" name that mode.

1. kernel contract (method of tests/test_live_rows_gpu.py) for the entry points that newly honour a count: first_layer_fwd
   in both forms, ln_act_bwd_first at every waves-per-row form, point_valid, and the segmented pool backward's pad-row
   zero fill in fp32, sx8 and scalar mode;
2. one captured first_layer_fwd + ln_act_bwd_first pair follows a new value of the same count tensor on replay;
3. forward_packed(tail="skip") on a NaN tail equals tail="compute" on a zero tail bit for bit: outputs, all 76 parameter
   gradients, point_features[:live]; a NaN cotangent tail; NaN-poisoned allocator memory; the routes that take the count
   and the ones that fall back;
4. skip mode against the golden file and, in fp32 (a fallback), against the decision-frozen fp64 oracle;
5. one captured train.py-shaped step with both tails skipped, replayed over batches of other point counts, equals eager
   tail="compute" steps bit for bit;
6. the interface on the device; 7. (not gpu) the interface on the host.
"""
import copy
import inspect
import os
import re

import numpy as np
import pytest
import torch

import helpers as H  # noqa: E402
import test_packed_capacity_gpu as TC  # noqa: E402
import test_packed_gpu as TP  # noqa: E402
from test_live_rows_gpu import (NAN, SENT, _capture, _contract, _lives, _precision, _ptrs, _r256, _rand, _sent,  # noqa: E402,F401
                                _tail, device_rng)
from test_packed_gpu import OUT_KEYS, TOL, TOL_OUT, dev, mode  # noqa: E402,F401

gpu = pytest.mark.gpu
RELU, GELU = 1, 2


# ---------------------------------------------------------------------------------------------------------------------
# 1. kernel contract
# ---------------------------------------------------------------------------------------------------------------------
def _first_layer_fn(R, K, D, act):
    from wf3d import ops
    lib, p, st, check = _ptrs()

    def fn(inp, cnt):
        z, mu, rs, h = _sent(R, D), _sent(R), _sent(R), _sent(R, D)
        x, W = inp["x"], inp["W"]
        with ops.live_rows(cnt):
            check(lib.wf3d_first_layer_fwd(p(x), R, K, x.stride(0), p(W), W.stride(0), p(inp["bias"]), D, p(inp["gamma"]),
                                           p(inp["beta"]), act, 1e-5, p(z), p(mu), p(rs), p(h), st()), "first_layer_fwd")
        return {"z": z, "mu": mu, "rs": rs, "h": h}
    return fn


@gpu
@pytest.mark.parametrize("K,D,act", [(8, 512, RELU), (8, 1024, RELU), (5, 264, GELU), (8, 512, GELU)],
                         ids=["fast512", "fast1024", "general264", "general512"])
def test_contract_first_layer_fwd(K, D, act):
    """FAST: K = 8, D a multiple of 512, ReLU (one and two column slots); the general form: K = 5, D = 264, and the
    FAST shape with another activation.  R = 1280 rows: five 256-row tiles, fewer than the grid's row stride and, with
    R = 5000, more (a workgroup then walks several rows and prefetches past the extent)."""
    for R in (1280, 5000):
        inputs = {"x": _rand(R, K, seed=1), "W": _rand(D, K, seed=2), "bias": _rand(D, seed=3), "gamma": _rand(D, seed=4),
                  "beta": _rand(D, seed=5)}
        _contract(f"first_layer_fwd K={K} D={D} R={R}", R, inputs, {"x"}, _first_layer_fn(R, K, D, act),
                  {"z", "mu", "rs", "h"}, _lives(R) if R == 1280 else [0, 257, R - 1])


def _bwd_first_fn(R, K, D):
    from wf3d import ops
    lib, p, st, check = _ptrs()

    def fn(inp, cnt):
        trio, dW = _sent(3, D), _sent(D, K)
        ws = torch.empty(lib.wf3d_ln_act_bwd_first_ws_bytes(R, D), dtype=torch.uint8, device=dev())
        x = inp["x"]
        with ops.live_rows(cnt):
            check(lib.wf3d_ln_act_bwd_first(p(inp["dh"]), p(inp["z"]), p(x), R, D, K, x.stride(0), p(inp["mu"]), p(inp["rs"]),
                                            p(inp["gamma"]), p(inp["beta"]), RELU, p(trio[0]), p(trio[1]), p(trio[2]), p(dW),
                                            p(ws), ws.numel(), st()), "ln_act_bwd_first")
        return {"trio": trio, "dW": dW}
    return fn


@gpu
@pytest.mark.parametrize("K,D", [(5, 264), (8, 512), (8, 1024), (3, 256)], ids=["wpr2-264", "wpr2-512", "wpr4-1024", "wpr1-256"])
def test_contract_ln_act_bwd_first(K, D):
    """One, two and four waves per row.  All four outputs are reductions over rows: bit-equal to the count-less call on a
    zero tail (dh = 0 rows add exact zeros), all-zero at live = 0."""
    R = 1280
    inputs = {"dh": _rand(R, D, seed=1), "z": _rand(R, D, seed=2), "x": _rand(R, K, seed=3), "mu": _rand(R, seed=4, scale=0.1),
              "rs": _rand(R, seed=5).abs() + 0.5, "gamma": _rand(D, seed=6), "beta": _rand(D, seed=7)}
    _contract(f"ln_act_bwd_first K={K} D={D}", R, inputs, {"dh", "z", "x", "mu", "rs"}, _bwd_first_fn(R, K, D), set())


@gpu
def test_contract_point_valid():
    from wf3d import ops
    lib, p, st, check = _ptrs()
    R = 1280
    x = _rand(R, 8, seed=1)
    x[5] = 0.0
    x[300:310] = 0.0

    def fn(inp, cnt):
        valid = _sent(R)
        with ops.live_rows(cnt):
            check(lib.wf3d_point_valid(p(inp["x"]), R, 8, p(valid), st()), "point_valid")
        return {"valid": valid}
    _contract("point_valid", R, {"x": x}, {"x"}, fn, {"valid"})


def _split3(live):
    """`live` rows over three clouds, none on a 256-row boundary where that is possible; a cloud may have no rows."""
    a = live * 3 // 5
    b = (live - a) // 3
    return [a, b, live - a - b]


@gpu
@pytest.mark.parametrize("C", [64, 48, 6])
def test_contract_pool4_seg_bwd(C):
    """Capacity 1280 (chunk_rows 256), three clouds whose rows sum to `live`: the pad rows live .. 1279 span up to five pad
    chunks that start at `live`, so their boundaries are no multiples of 256 and R256 falls inside the first one.  fp32
    and sx8 for C = 64 and 48 (16-byte rows), the scalar kernel for C = 6.  Without a count every pad row is written as
    zeros; under the layout's own count (rows[B]) the rows >= R256 keep the sentinel, the rows below are bit-equal."""
    from wf3d import ops
    lib, p, st, check = _ptrs()
    cap, B = 1280, 3
    assert ops.chunk_rows_of(cap) == 256
    g = torch.Generator().manual_seed(C)
    pf = torch.randn(cap, C, generator=g).to(dev())
    valid0 = (torch.rand(cap, generator=g) > 0.2).float().to(dev())
    direct0 = torch.randn(cap, C, generator=g).to(dev())
    cot = torch.randn(B, 4 * C, generator=g).to(dev())
    cots = (cot[:, :C], cot[:, C:2 * C], cot[:, 2 * C:3 * C], cot[:, 3 * C:])

    def run(lay, po, valid, direct, sx8, cnt):
        dpf = _sent(cap, C)
        fn = lib.wf3d_pool4_seg_bwd_sx8 if sx8 else lib.wf3d_pool4_seg_bwd
        with ops.live_rows(cnt):
            check(fn(p(valid), p(po.cnt), p(po.arg_m), p(po.arg_u), p(cots[0]), p(cots[1]), 4 * C, p(cots[2]), p(cots[3]), 4 * C,
                     p(direct), p(lay.d_rows), p(lay.d_chunks), B, lay.M_abi, lay.M_pad, lay.nchunk_bwd, lay.chunk_rows, C,
                     p(dpf), st()), "pool4_seg_bwd")
        return dpf

    for live in _lives(cap):
        counts = _split3(live)
        lay = ops.DevicePackedLayout(B, cap, dev()).build(torch.tensor(counts, device=dev()))
        chunks = lay.d_chunks.cpu().numpy().reshape(-1, 4)
        pads = chunks[(chunks[:, 0] < 0) & (chunks[:, 3] > chunks[:, 2])]
        assert lay.d_rows.tolist()[-1] == live and (live == cap or pads[0, 2] == live)
        if live in (1, 257):
            assert len(pads) >= 4 and pads[1, 2] % 256 != 0                  # several pad chunks, odd boundaries
        r = _r256(live, cap)
        po = ops.pool4_seg_fwd(pf, _tail(valid0, r, 0.0), lay)
        for sx8 in [False] + ([True] if C % 8 == 0 else []):
            for use_direct in (False, True):
                want = run(lay, po, _tail(valid0, r, 0.0), _tail(direct0, r, 0.0) if use_direct else None, sx8, None)
                got = run(lay, po, _tail(valid0, r, NAN), _tail(direct0, r, NAN) if use_direct else None, sx8,
                          lay.d_rows[B:B + 1])
                torch.cuda.synchronize()
                tag = (C, live, sx8, use_direct)
                assert not bool((want == SENT).any()), tag                    # the count-less call writes every row
                assert torch.equal(got[:r].view(torch.int32), want[:r].view(torch.int32)), tag
                assert not bool(got[live:r].view(torch.int32).any()), tag     # dead rows below R256: exact zeros
                assert bool((got[r:] == SENT).all()), (tag, "tail rows written")
                assert not bool(torch.isnan(got[:r]).any()) or sx8, tag


@gpu
def test_pool4_seg_fwd_never_reads_a_pad_row():
    """wf3d_pool4_seg_fwd takes no count: it reaches rows through the clouds' chunks only.  NaN in every pad row of
    point_features and valid changes nothing, with a count set or not."""
    from wf3d import ops
    cap, C = 1280, 64
    lay = ops.DevicePackedLayout(3, cap, dev()).build(torch.tensor([300, 1, 200], device=dev()))
    pf, valid = _rand(cap, C, seed=1), (_rand(cap, seed=2) > -0.5).float()
    want = ops.pool4_seg_fwd(_tail(pf, 501, 0.0), _tail(valid, 501, 0.0), lay)
    for cnt in (None, lay.d_rows[3:4]):
        with ops.live_rows(cnt):
            got = ops.pool4_seg_fwd(_tail(pf, 501, NAN), _tail(valid, 501, NAN), lay)
        for f in ("masked", "unmasked", "arg_m", "arg_u", "cnt", "nvalid"):
            assert torch.equal(getattr(got, f), getattr(want, f)), f


# ---------------------------------------------------------------------------------------------------------------------
# 2. same pointer, new value
# ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_captured_first_layer_pair_follows_the_count_tensor():
    R, K, D = 1280, 8, 512
    x, W, bias, gamma, beta = _rand(R, K, seed=1), _rand(D, K, seed=2), _rand(D, seed=3), _rand(D, seed=4), _rand(D, seed=5)
    dh = _rand(R, D, seed=6)
    fwd, bwd = _first_layer_fn(R, K, D, RELU), _bwd_first_fn(R, K, D)
    base = {"x": x, "W": W, "bias": bias, "gamma": gamma, "beta": beta}
    full = fwd(base, None)
    cnt = torch.tensor([300], dtype=torch.int32, device=dev())
    from wf3d import ops
    lib, p, st, check = _ptrs()
    z, mu, rs, h = _sent(R, D), _sent(R), _sent(R), _sent(R, D)
    trio, dW = _sent(3, D), _sent(D, K)
    ws = torch.empty(lib.wf3d_ln_act_bwd_first_ws_bytes(R, D), dtype=torch.uint8, device=dev())

    def fn():
        with ops.live_rows(cnt):
            check(lib.wf3d_first_layer_fwd(p(x), R, K, x.stride(0), p(W), W.stride(0), p(bias), D, p(gamma), p(beta), RELU,
                                           1e-5, p(z), p(mu), p(rs), p(h), st()), "first_layer_fwd")
            check(lib.wf3d_ln_act_bwd_first(p(dh), p(z), p(x), R, D, K, x.stride(0), p(mu), p(rs), p(gamma), p(beta), RELU,
                                            p(trio[0]), p(trio[1]), p(trio[2]), p(dW), p(ws), ws.numel(), st()),
                  "ln_act_bwd_first")
    graph, _ = _capture(fn)
    sums = {}
    for live in (300, 0, 700, 1280, 1):
        cnt.fill_(live)
        for t in (z, mu, rs, h, trio, dW):
            t.fill_(SENT)
        graph.replay()
        torch.cuda.synchronize()
        r = _r256(live, R)
        for k, t in (("z", z), ("mu", mu), ("rs", rs), ("h", h)):
            assert torch.equal(t[:r], full[k][:r]) and bool((t[r:] == SENT).all()), (live, k)
        want = bwd(dict(base, dh=_tail(dh, r, 0.0), z=full["z"], mu=full["mu"], rs=full["rs"]), None)
        assert torch.equal(trio, want["trio"]) and torch.equal(dW, want["dW"]), live
        sums[r] = dW.clone()
    assert not bool(sums[0].any()) and not torch.equal(sums[512], sums[1280])      # a shorter extent shows in the sums


# ---------------------------------------------------------------------------------------------------------------------
# 3. model level: skip == compute, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
class _enc_spy:
    """Records what functional._encoder_live decided, so that a silent fallback cannot pass for the skip path."""

    def __enter__(self):
        from wf3d import functional
        self.f, self.orig, self.seen = functional, functional._encoder_live, []

        def spy(layout, routes, tail):
            out = self.orig(layout, routes, tail)
            self.seen.append((tail, out is not None, tuple((r.fwd, r.wgrad) for r in routes)))
            return out
        functional._encoder_live = spy
        return self

    def __exit__(self, *exc):
        self.f._encoder_live = self.orig

    def took(self):
        return [(t, hit) for t, hit, _ in self.seen]


CAP = 2048
# name -> (point counts, how they are passed: a host list, or the dtype of a device tensor)
POINT_COUNTS = {"ragged": ([300, 1, 200], "host"), "boundary": ([256, 256, 256], torch.int64), "257": ([255, 1, 1], torch.int32),
                "full": ([1000, 1000, 48], "host"), "one-row": ([1, 0, 0], torch.int64), "no-rows": ([0, 0, 0], torch.int32)}
DEFAULT_ROUTES = (("first", "first"),) + (("split", "tn"),) * 4


def _batch(pcounts, fill, seed=3):
    """[CAP, 8]: the clouds, zeros up to R256 (dead rows of the last live tile), `fill` from R256 on."""
    live = sum(pcounts)
    g = torch.Generator().manual_seed(seed)
    pts = torch.zeros(CAP, 8)
    pts[:live] = torch.randn(live, 8, generator=g)
    pts[_r256(live, CAP):] = fill
    return pts.to(dev())


def _counts_arg(pcounts, how):
    return list(pcounts) if how == "host" else torch.tensor(pcounts, dtype=how, device=dev())


def _model_run(m, pts, counts, tc, tail):
    m.zero_grad(set_to_none=True)
    if tail is not None:                        # None: whatever the model holds (the default)
        m.set_packed_tail(tail)
    out = m.forward_packed(pts, counts, tc, capacity=CAP)
    TC._loss(out).backward()
    return out, TC._grads(m)


def _assert_same(a, b, ngrads=76):
    """ngrads = None: whatever set of parameters took a gradient (eval mode: the edge head's counts depend on the data)."""
    (oa, ga), (ob, gb) = a, b
    for k in OUT_KEYS:
        assert torch.equal(oa[k], ob[k]), k
        assert bool(torch.isfinite(ob[k]).all()), k
    assert oa["edge_indices"] == ob["edge_indices"]
    assert ("point_status" in oa) == ("point_status" in ob)
    if "point_status" in oa:
        assert torch.equal(oa["point_status"], ob["point_status"])
    assert set(ga) == set(gb) and (ngrads is None or len(ga) == ngrads)
    for n in ga:
        assert bool(torch.isfinite(gb[n]).all()), n
        assert torch.equal(ga[n], gb[n]), n


@gpu
@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("which", list(POINT_COUNTS))
def test_skip_equals_compute(precision, train, which):
    """Default widths (8 -> 512 -> 1024 -> 2048 -> 1024 -> 512) at capacity 2,048: the fused first layer in its FAST form and
    four split Linears with TN-kernel wgrads, all under the count.  compute sees zeros behind the clouds, skip NaN from
    R256 on."""
    pcounts, how = POINT_COUNTS[which]
    live = sum(pcounts)
    m = TC._model()
    m.train(train)
    tc = torch.tensor([6, 2, 4], device=dev()) if train else None
    with _precision(precision), _enc_spy() as spy:
        a = _model_run(m, _batch(pcounts, 0.0), _counts_arg(pcounts, how), tc, "compute")
        b = _model_run(m, _batch(pcounts, NAN), _counts_arg(pcounts, how), tc, "skip")
        with torch.no_grad():
            pa = m.encoder.set_packed_tail("compute").encode_packed(_batch(pcounts, 0.0), _counts_arg(pcounts, how), capacity=CAP)
            pb = m.encoder.set_packed_tail("skip").encode_packed(_batch(pcounts, NAN), _counts_arg(pcounts, how), capacity=CAP)
    torch.cuda.synchronize()
    assert spy.took() == [("compute", False), ("skip", True)] * 2, spy.seen
    assert all(r == DEFAULT_ROUTES for _, _, r in spy.seen), spy.seen
    _assert_same(a, b, 76 if train else None)
    assert pb[1].shape == (CAP, 512)
    for x, y in zip(pa, pb):
        assert torch.equal(x[:live] if x.shape[0] == CAP else x, y[:live] if y.shape[0] == CAP else y)
    assert not bool(torch.isnan(pb[1][:_r256(live, CAP)]).any())
    if how != "host":
        assert b[0]["point_status"].tolist() == [2 if 0 in pcounts else 0]


def _encoder_run(enc, pts, counts, cots, tail):
    for p_ in enc.parameters():
        p_.grad = None
    outs = enc.set_packed_tail(tail).encode_packed(pts, counts, capacity=CAP)
    torch.autograd.backward(list(outs), list(cots))
    return outs, {n: p_.grad for n, p_ in enc.named_parameters() if p_.grad is not None}


def _encoder_same(a, b, live):
    (oa, ga), (ob, gb) = a, b
    assert torch.equal(oa[0], ob[0]) and torch.equal(oa[2], ob[2]) and torch.equal(oa[1][:live], ob[1][:live])
    assert set(ga) == set(gb) and ga
    for n in ga:
        assert bool(torch.isfinite(gb[n]).all()), n
        assert torch.equal(ga[n], gb[n]), n


def _encoder_cots(C, live, fill, seed=5):
    g = torch.Generator().manual_seed(seed)
    cg, cup = torch.randn(3, C, generator=g).to(dev()), torch.randn(3, 2 * C, generator=g).to(dev())
    cpf = torch.zeros(CAP, C)
    cpf[:live] = torch.randn(live, C, generator=g)
    cpf[_r256(live, CAP):] = fill
    return cg, cpf.to(dev()), cup


@gpu
@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
def test_skip_with_a_nan_tail_in_the_point_feature_cotangent(precision):
    """A gradient arrives for point_features itself: its rows >= R256 are not read under skip."""
    from models.PointNetEncoder import PointNetEncoder
    pcounts = [300, 1, 200]
    live = sum(pcounts)
    torch.manual_seed(1)
    enc = PointNetEncoder().to(dev()).train()
    with _precision(precision), _enc_spy() as spy:
        a = _encoder_run(enc, _batch(pcounts, 0.0), pcounts, _encoder_cots(512, live, 0.0), "compute")
        b = _encoder_run(enc, _batch(pcounts, NAN), torch.tensor(pcounts, device=dev()), _encoder_cots(512, live, NAN), "skip")
    assert spy.took() == [("compute", False), ("skip", True)], spy.seen
    _encoder_same(a, b, live)
    assert len(a[1]) == 28                      # 18 of the per-point MLP, 10 of the fusion MLP


@gpu
@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
def test_skip_on_poisoned_memory(precision):
    """As tests/test_live_rows_gpu.py::test_skip_on_poisoned_memory: the allocator hands out NaN-filled blocks, so a tail
    row that is read (never having been written under skip) would show."""
    pcounts, tc = [300, 1, 200], torch.tensor([6, 2, 4], device=dev())
    m = TC._model()
    pc = torch.tensor(pcounts, device=dev())

    def run(fill, tail):
        junk = torch.full((256 << 20,), fill, dtype=torch.float32, device=dev())      # 1 GiB handed back to the cache
        del junk
        return _model_run(m, _batch(pcounts, NAN if tail == "skip" else 0.0), pc, tc, tail)

    with _precision(precision), _enc_spy() as spy:
        torch.cuda.synchronize()
        bad = run(NAN, "skip")
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        good = run(0.0, "compute")
        torch.cuda.synchronize()
    assert spy.took() == [("skip", True), ("compute", False)], spy.seen
    _assert_same(good, bad)


@gpu
def test_skip_in_fp32_falls_back_and_still_equals():
    """precision fp32: every Linear runs wf3d_gemm, which sees no count, so skip computes the tail (and needs it finite)."""
    pcounts, tc = [300, 1, 200], torch.tensor([6, 2, 4], device=dev())
    m = TC._model()
    with _precision("fp32"), _enc_spy() as spy:
        a = _model_run(m, _batch(pcounts, 0.0), pcounts, tc, "compute")
        b = _model_run(m, _batch(pcounts, 7.0), torch.tensor(pcounts, device=dev()), tc, "skip")
    assert spy.took() == [("compute", False), ("skip", False)], spy.seen
    assert all(r[0] == ("fp32", "fp32") for _, _, r in spy.seen), spy.seen
    b[0].pop("point_status")
    _assert_same(a, b)


# hidden widths -> (takes the count, the (fwd, wgrad) of every Linear at 2,048 rows in bf16x3)
WIDTH_SETS = {
    # 2048 columns are more than the fused first layer takes (first_layer_ok): Linear 0 is an fp32 GEMM
    "first-refused": ([2048, 512], False, (("fp32", "fp32"), ("split", "tn"), ("split", "tn"))),
    # 100 is no multiple of 8: Linear 1 forms an fp32 wgrad (and dgrad), the output Linear runs fp32
    "fp32-wgrad": ([512, 100], False, (("first", "first"), ("split", "fp32"), ("fp32", "fp32"))),
    # 264 columns: the general first-layer form; 264 and 200 are no multiples of 256 / 128, which the TN kernel tiles:
    # the wgrads of Linears 1 and 2 take split_transpose + the NT GEMM
    "general-transposes": ([264, 200], True, (("first", "first"), ("split", "transposes"), ("split", "transposes"))),
}


@gpu
@pytest.mark.parametrize("which", list(WIDTH_SETS))
def test_skip_equals_compute_at_other_widths(which):
    """PointNetEncoder(hidden_dims=...) sets that leave the default routes (named in WIDTH_SETS): two fall back to
    computing the tail, one takes the count through the general first-layer kernel and the "transposes" wgrad."""
    from models.PointNetEncoder import PointNetEncoder
    dims, takes, routes = WIDTH_SETS[which]
    pcounts = [300, 1, 200]
    live = sum(pcounts)
    torch.manual_seed(2)
    enc = PointNetEncoder(hidden_dims=dims).to(dev()).train()
    fill = NAN if takes else 3.0                        # a fallback computes the tail: it has to be finite
    with _precision("bf16x3"), _enc_spy() as spy:
        a = _encoder_run(enc, _batch(pcounts, 0.0), pcounts, _encoder_cots(512, live, 0.0), "compute")
        b = _encoder_run(enc, _batch(pcounts, fill), pcounts, _encoder_cots(512, live, NAN if takes else 0.0), "skip")
    assert spy.took() == [("compute", False), ("skip", takes)], spy.seen
    assert all(r == routes for _, _, r in spy.seen), spy.seen
    _encoder_same(a, b, live)


# ---------------------------------------------------------------------------------------------------------------------
# 4. golden file and fp64 oracle
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mode", TP.FORCED[:2], indirect=True, ids=lambda m: m[0])
def test_capacity_forward_vs_golden_skip(mode):
    """tests/test_packed_capacity_gpu.py::test_capacity_forward_vs_golden with tail="skip": same golden file and bounds.
    bf16x3 takes the count and gets a NaN tail from R256 on; fp32 falls back, where the tail has to be finite."""
    gold, model, clouds, points, pcounts, counts, V, seed = TP.build_packed()
    live = sum(pcounts)
    cap = -(-live // 256) * 256 + 512
    pts = TC._pad_to(points, cap)
    if mode != "fp32":
        pts[_r256(live, cap):] = NAN
    with _enc_spy() as spy:
        out = model.set_packed_tail("skip").forward_packed(pts, torch.tensor(pcounts, device=dev()), counts.to(dev()),
                                                           capacity=cap)
    assert spy.took() == [("skip", mode != "fp32")], spy.seen
    assert out["point_status"].tolist() == [0]
    TP._check_outputs(out, gold, TOL_OUT)
    cot = TP._golden_cotangents(out, seed)
    loss = sum((out[k] * cot[k].to(dev())).sum() for k in cot)
    loss.backward()
    assert abs(loss.item() - float(gold["out.loss"])) < 1e-4 * max(1.0, abs(float(gold["out.loss"])))
    bad = H.check_grad_summaries(gold, [(n, p.grad) for n, p in model.named_parameters()], TP.TOL_GRAD)
    assert not bad, bad


@gpu
def test_capacity_frozen_gradients_fp32_elementwise_skip(monkeypatch):
    """tests/test_packed_capacity_gpu.py::test_capacity_frozen_gradients_fp32_elementwise, unchanged in method, with
    tail="skip".  fp32 falls back to computing the tail: the bound holds in every mode."""
    from models.PointCloudToWireframe import PointCloudToWireframe
    plain, calls = PointCloudToWireframe.forward_packed, []

    def with_capacity(self, points, point_counts, target_vertex_counts=None):
        calls.append(1)
        pc = torch.tensor(point_counts, device=points.device)
        return plain(self.set_packed_tail("skip"), TC._pad_to(points, 512), pc, target_vertex_counts, capacity=512)

    monkeypatch.setattr(PointCloudToWireframe, "forward_packed", with_capacity)
    with _enc_spy() as spy:
        fwd, errs, seed = TP._run_frozen("fp32", [96, 37, 160], 12, [12, 2, 7], 1, False, 32)
    assert calls and spy.seen and all(t == ("skip", False) for t in spy.took()), spy.seen
    TP._report("fp32 capacity skip", fwd, errs, seed)
    for k, (a, b) in fwd.items():
        assert a < TOL and b < TOL, (k, a, b)
    assert len(errs) == 76
    bad = [(n, e) for n, e in errs.items() if not e <= TOL]
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------
# 5. one capture
# ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_one_captured_skip_step_equals_eager_compute_steps(device_rng):
    """A train.py-shaped step (padded edge head tail="skip", encoder tail="skip", device dropout seeds, capturable
    ClipAdam) captured once with point counts A and replayed on batches of other point and vertex counts, one of which
    fills the capacity: parameters and gradients equal eager steps with both tails computed, bit for bit."""
    from losses.WireframeLoss import WireframeLoss
    from models.PointCloudToWireframe import PointCloudToWireframe
    from wf3d import config
    from wf3d.optim import ClipAdam
    from wf3d.packed import pack_into
    from wf3d.random import default_generator
    from wf3d.targets import train_targets
    B, V, cap = 3, 32, 1536
    assert cap >= config.SPLIT_MIN_ROWS and config.precision() in ("bf16x3", "bf16")
    torch.manual_seed(0)
    gen = default_generator(dev())
    model = PointCloudToWireframe(8, V).to(dev()).set_dropout(0.1).train().set_edge_layout("padded", tail="skip")
    twin = copy.deepcopy(model).set_edge_layout("padded", tail="compute")
    model.set_packed_tail("skip")
    assert twin.encoder._packed_tail == "compute"
    rng = np.random.default_rng(1)
    pcs = [[300, 1, 700], [10, 1200, 257], [512, 1000, 24], [1, 1, 1], [255, 1, 256], [700, 300, 400]]
    assert sum(pcs[2]) == cap
    batches = []
    for pc in pcs:
        cnt = rng.integers(4, V + 1, size=B).tolist()
        vs = [rng.standard_normal((c, 3)).astype(np.float32) for c in cnt]
        es = [np.stack([np.arange(c - 1), np.arange(1, c)], 1) for c in cnt]
        t = train_targets(vs, es, V, device=dev(), full_width=True)
        t["clouds"] = [torch.from_numpy(rng.standard_normal((n, 8)).astype(np.float32)) for n in pc]
        batches.append(t)
    tkeys = ("vertices", "vertex_existence", "edge_labels", "vertex_counts")
    static = {k: batches[0][k].clone() for k in tkeys}
    points = torch.zeros(cap, 8, device=dev())
    counts = torch.zeros(B, dtype=torch.int64, device=dev())
    crit = WireframeLoss(vertex_weight=3.0, edge_weight=1.0, existence_weight=1.5, assignment="device")

    def load(bt):
        pack_into(points, counts, bt["clouds"])
        for k in tkeys:
            static[k].copy_(bt[k])

    def step(m, opt):
        opt.zero_grad()
        out = m.forward_packed(points, counts, static["vertex_counts"], capacity=cap)
        res = crit(out, static)
        res["total_loss"].backward()
        opt.step()

    def setup(m):
        return ClipAdam(m.parameters(), lr=1e-3, weight_decay=1e-6, max_norm=1.0, norm_params=m.parameters, capturable=True)

    opt, opt2 = setup(model), setup(twin)
    load(batches[0])
    start = gen.get_state()
    torch.manual_seed(2)
    with _enc_spy() as spy:
        graph, _ = _capture(lambda: step(model, opt))
        assert spy.seen and all(t == ("skip", True) for t in spy.took()), spy.seen
        gen.set_state(start)
        torch.manual_seed(2)
        n0 = len(spy.seen)
        for _ in range(2):
            step(twin, opt2)
        assert all(t == ("compute", False) for t in spy.took()[n0:]), spy.seen
    named2 = dict(twin.named_parameters())
    for k, bt in enumerate(batches[1:] + batches[:2]):
        load(bt)
        before = gen.get_state()
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")                       # a host read of the counts would raise here
        try:
            graph.replay()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        after = gen.get_state()
        gen.set_state(before)
        step(twin, opt2)
        torch.cuda.synchronize()
        assert torch.equal(gen.get_state(), after)
        for n, p_ in model.named_parameters():
            assert torch.equal(p_, named2[n]), (k, n)
            assert (p_.grad is None) == (named2[n].grad is None) and (p_.grad is None or torch.equal(p_.grad, named2[n].grad)), (k, n)
            assert bool(torch.isfinite(p_).all()), (k, n)


# ---------------------------------------------------------------------------------------------------------------------
# 6. interface, on the device
# ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_interface_on_the_device():
    pcounts, tc = [300, 1, 200], torch.tensor([6, 2, 4], device=dev())
    m = TC._model()
    pts = _batch(pcounts, 0.0)
    with pytest.raises(ValueError, match="'compute' or 'skip'"):
        m.set_packed_tail("drop")
    with pytest.raises(ValueError, match="'compute' or 'skip'"):
        m.encoder.set_packed_tail(None)
    with _enc_spy() as spy:
        a = _model_run(m, pts, pcounts, tc, None)                      # a model nobody set a tail on
        b = _model_run(m, pts, pcounts, tc, "compute")
    assert spy.took() == [("compute", False)] * 2
    _assert_same(a, b)
    m.set_packed_tail("skip")
    with pytest.raises(ValueError, match="needs a capacity"):
        m.forward_packed(pts[:501].contiguous(), pcounts, tc)
    with pytest.raises(ValueError, match="needs a capacity"):
        m.encoder.encode_packed(pts[:501].contiguous(), pcounts)
    out = m.set_packed_tail("compute").forward_packed(pts[:501].contiguous(), pcounts, tc)      # and back
    assert bool(torch.isfinite(out["vertices"]).all())


# ---------------------------------------------------------------------------------------------------------------------
# 7. interface, on the host (no GPU needed)
# ---------------------------------------------------------------------------------------------------------------------
def test_interface_on_the_host():
    """The tail checks precede the device check: they raise on CPU tensors.  The mode is a setting of the module
    (set_packed_tail, like set_edge_layout's tail) and not an argument: tests/test_packed_capacity.py holds the
    parameter lists of encode_packed / forward_packed to exactly (points, point_counts[, target_vertex_counts],
    capacity), so both signatures are asserted unchanged here.  The ABI version is unchanged too."""
    from models.PointCloudToWireframe import PointCloudToWireframe
    from models.PointNetEncoder import PointNetEncoder
    m = PointCloudToWireframe(8, 6)
    assert m.encoder._packed_tail == "compute"
    with pytest.raises(ValueError, match="'compute' or 'skip'"):
        m.set_packed_tail("drop")
    with pytest.raises(ValueError, match="'compute' or 'skip'"):
        m.encoder.set_packed_tail("")
    assert m.encoder._packed_tail == "compute"                          # a refused value changes nothing
    assert m.set_packed_tail("skip") is m and m.encoder._packed_tail == "skip"
    with pytest.raises(ValueError, match="needs a capacity"):
        m.forward_packed(torch.zeros(12, 8), [5, 7])
    with pytest.raises(ValueError, match="needs a capacity"):
        m.encoder.encode_packed(torch.zeros(12, 8), [5, 7])
    with pytest.raises(RuntimeError, match="no CPU fallback"):        # with a capacity the call goes on to the device check
        m.forward_packed(torch.zeros(256, 8), [5, 7], capacity=256)
    enc = PointNetEncoder()
    assert enc.set_packed_tail("skip") is enc and enc.set_packed_tail("compute") is enc
    with pytest.raises(RuntimeError, match="no CPU fallback"):        # "compute" without a capacity: as before
        enc.encode_packed(torch.zeros(12, 8), [5, 7])
    sig = inspect.signature(PointNetEncoder.encode_packed).parameters
    assert list(sig) == ["self", "points", "point_counts", "capacity"] and sig["capacity"].default is None
    sig = inspect.signature(PointCloudToWireframe.forward_packed).parameters
    assert list(sig) == ["self", "points", "point_counts", "target_vertex_counts", "capacity"]
    assert sig["capacity"].default is None and sig["target_vertex_counts"].default is None
    for cls in (PointNetEncoder, PointCloudToWireframe):
        assert list(inspect.signature(cls.set_packed_tail).parameters) == ["self", "tail"]
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "include", "wf3d.h")).read()
    assert re.search(r"^#define\s+WF3D_VERSION\s+105\b", header, re.M)
    doc = header[header.index("LIVE ROW COUNT"):]
    honoured, rest = doc[:doc.index("EVERY OTHER")], doc[doc.index("EVERY OTHER"):doc.index("wf3d_set_live_rows(const")]
    for name in ("wf3d_first_layer_fwd", "wf3d_ln_act_bwd_first", "wf3d_point_valid", "wf3d_pool4_seg_bwd", "wf3d_pool4_seg_bwd_sx8"):
        assert name in honoured and name not in rest, name
