"""Train-mode dropout at the encoder's sites mlp.{4i+3}: the fused first-layer kernels against the host mask, and
PointNetEncoder on every route against the fp64 model fed the masks of the seed the forward recorded.

  - wf3d_first_layer_fwd_drop: z, mu, rs bit-equal to the call without a mask; the unpacked sx8 h exactly zero where the
    host drops (oracle/dropout.py recomputes every bit), the p = 0 value times the fp32 scale elsewhere
    (assert_masked_close and its bound, tests/test_dropout_gpu.py); under a live-row count; with device seed words.
  - wf3d_ln_act_bwd_first_drop: equals the p = 0 call on the host-masked dh (the comparison of test_dropout_gpu's
    ln_act_bwd test).
  - PointNetEncoder.encode / encode_packed in train mode with site probabilities (0.05, 0.1, 0.2, 0.3): all three outputs
    and every element of every parameter gradient against tests/dropout_sites_model.py under the replayed masks and
    the kernels' own decisions, at the bounds of tests/test_encoder_cotangents_gpu.py (TOL, TOL_X3_FORCED; bf16: the
    recorded bounds of tests/test_precision_bf16_gpu.py).  Every case asserts its routes on the autograd node; together
    they cover forward first / split / fp32, wgrad first / tn / transposes / fp32, dgrad split / fp32.
  - plumbing: eval() and p = 0 draw nothing and are today's bits; p = 1 raises naming the site; the forward-only stream
    path is left while a site is active; device seed words serve four sites.

Each case prints its worst errors (pytest -s)."""
import contextlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import dropout_sites_model as M  # noqa: E402
import enc_cases as E  # noqa: E402
import helpers as H  # noqa: E402
from helpers import unpack_sx8  # noqa: E402
from oracle import dropout as D  # noqa: E402
from test_dropout_gpu import PS, SEEDS, _bwd_pair, _close, assert_masked_close, host_keep, rnd  # noqa: E402
from test_encoder_cotangents_gpu import TOL, TOL_X3_FORCED  # noqa: E402

SITE_PS = (0.05, 0.1, 0.2, 0.3)
DRAWS = 32


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from wf3d import ops as o
    o._lib.load()
    return o


# ----------------------------------------------------------------------------------------------------------------------
# the first-layer kernels
# ----------------------------------------------------------------------------------------------------------------------
R_, D_ = 2500, 512           # 625 workgroups of four rows, the last row group ragged against the 4096-block grid stride


def first_inputs(K):
    x = rnd(R_, K, seed=1)
    W, b = rnd(D_, K, seed=2, scale=0.5), 0.1 * rnd(D_, seed=3)
    gamma, beta = 1 + 0.2 * rnd(D_, seed=4), 0.1 * rnd(D_, seed=5)
    return x, W, b, gamma, beta


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("K", [3, 8])
def test_first_layer_fwd_mask_is_the_host_mask(ops, K, p, seed):
    x, W, b, gamma, beta = first_inputs(K)
    z0, mu0, rs0, h0 = ops.first_layer_fwd(x, W, b, gamma, beta, ops.ACT_RELU)
    z, mu, rs, h = ops.first_layer_fwd(x, W, b, gamma, beta, ops.ACT_RELU, drop_p=p, seed=seed)
    assert torch.equal(z, z0) and torch.equal(mu, mu0) and torch.equal(rs, rs0)
    hi, lo = unpack_sx8(h)
    hi0, lo0 = unpack_sx8(h0)
    keep = host_keep(seed, R_, D_, p)
    assert_masked_close(hi + lo, hi0 + lo0, keep, p, 3e-5)
    assert 0.5 * p < float((~keep).double().mean()) < 1.5 * p


def _fwd_into(ops, lib, x, W, b, gamma, beta, p, seed, fill):
    """wf3d_first_layer_fwd_drop into buffers pre-filled with `fill`: what the call leaves untouched stays visible."""
    z = torch.full((R_, D_), fill, device=dev())
    h = torch.full((R_, D_), fill, device=dev())
    mu, rs = torch.full((R_,), fill, device=dev()), torch.full((R_,), fill, device=dev())
    ops.check(lib.wf3d_first_layer_fwd_drop(ops._p(x), R_, x.shape[1], x.stride(0), ops._p(W), W.stride(0), ops._p(b), D_,
                                            ops._p(gamma), ops._p(beta), ops.ACT_RELU, ops.LN_EPS, p, seed, ops._p(z),
                                            ops._p(mu), ops._p(rs), ops._p(h), ops._stream()), "first_layer_fwd_drop")
    return z, mu, rs, h


@pytest.mark.parametrize("K", [3, 8])
def test_first_layer_fwd_drop_under_a_live_row_count(ops, K):
    """1300 live rows: the extent is 1536.  Rows at or past it are untouched, the rows below are the uncounted call's."""
    p, seed = 0.1, SEEDS[1]
    lib = ops._lib.load()
    x, W, b, gamma, beta = first_inputs(K)
    full = _fwd_into(ops, lib, x, W, b, gamma, beta, p, seed, -7.0)
    cnt = torch.tensor([1300], dtype=torch.int32, device=dev())
    with ops.live_rows(cnt):
        got = _fwd_into(ops, lib, x, W, b, gamma, beta, p, seed, -7.0)
    for a, f in zip(got, full):
        assert torch.equal(a[:1536], f[:1536])
        assert bool((a[1536:] == -7.0).all())
    assert not bool((full[0][1536:] == -7.0).any())


def test_first_layer_fwd_drop_with_device_seed_words(ops):
    from wf3d.random import seed_words
    p, seed = 0.5, SEEDS[1]
    x, W, b, gamma, beta = first_inputs(8)
    want = ops.first_layer_fwd(x, W, b, gamma, beta, ops.ACT_RELU, drop_p=p, seed=seed)
    words = torch.tensor([11, 22, seed - (1 << 32), 44, 55], dtype=torch.int32, device=dev())      # the same 32 bits
    with seed_words(words):
        got = ops.first_layer_fwd(x, W, b, gamma, beta, ops.ACT_RELU, drop_p=p, seed=2)
        same = ops.first_layer_fwd(x, W, b, gamma, beta, ops.ACT_RELU, drop_p=0.0, seed=2)       # p = 0 reads no word
    for a, w in zip(got, want):
        assert torch.equal(a, w)
    assert torch.equal(same[3], ops.first_layer_fwd(x, W, b, gamma, beta, ops.ACT_RELU)[3])
    assert not torch.equal(got[3], same[3])


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("K", [3, 8])
def test_ln_act_bwd_first_mask_is_the_host_mask(ops, K, p, seed):
    """The drop call on dh equals the p = 0 call on dh * keep * scale: dgamma, dbeta, dbias and the weight gradient."""
    x, W, b, gamma, beta = first_inputs(K)
    z, mu, rs, _ = ops.first_layer_fwd(x, W, b, gamma, beta, ops.ACT_RELU)
    dh = rnd(R_, D_, seed=20)

    def run(d, pp):
        return ops.ln_act_bwd_first(d, z, x, mu, rs, gamma, beta, ops.ACT_RELU, drop_p=pp, seed=seed)

    got, ref = _bwd_pair(run, dh, host_keep(seed, R_, D_, p), p)
    plain = run(dh.clone(), 0.0)
    for a, r, pl in zip(got, ref, plain):
        _close(a, r)
        assert not torch.equal(a, pl)
    assert got[3].shape == (D_, K)


# ----------------------------------------------------------------------------------------------------------------------
# PointNetEncoder in train mode against the fp64 model under the replayed masks
# ----------------------------------------------------------------------------------------------------------------------
FIRST = ("first", "first", None)
FP32_0 = ("fp32", "fp32", None)
FP32 = ("fp32", "fp32", "fp32")
TN, TR = ("split", "tn", "split"), ("split", "transposes", "split")

# id -> widths, (B, N) or packed counts, precision, SPLIT_MIN_ROWS (None: the default), the routes it must show, bounds
CASES = {
    # (a) widths whose wgrad takes the TN kernel (and, for the 64-wide output layer, the transposes)
    "a-tn":        dict(hidden=[256, 512], out=64, B=2, N=640, precision="bf16x3", min_rows=1, routes=[FIRST, TN, TR]),
    # (b) the "transposes" route on every Linear, three sites
    "b-transposes": dict(hidden=[64, 128, 64], out=40, B=2, N=100, precision="bf16x3", min_rows=1, routes=[FIRST, TR, TR, TR]),
    # (c) fp32 arithmetic, and a bf16x3 batch below SPLIT_MIN_ROWS: the same fp32 kernels, so the fp32 bound
    "c-fp32":      dict(hidden=[128, 64], out=32, B=2, N=100, precision="fp32", min_rows=1, routes=[FP32_0, FP32, FP32]),
    "c-x3-small":  dict(hidden=[128, 64], out=32, B=2, N=100, precision="bf16x3", min_rows=None, routes=[FP32_0, FP32, FP32],
                        tol=TOL),
    # (d) three input columns: the first-layer kernels' general (not FAST) form
    "d-din3":      dict(hidden=[64], out=40, B=2, N=100, din=3, precision="bf16x3", min_rows=1, routes=[FIRST, TR]),
    # (e) the input requires grad: layer 0 backward on the fp32 wgrad / dgrad, dx compared
    "e-dx":        dict(hidden=[128], out=256, B=2, N=48, precision="bf16x3", min_rows=1, want_dx=True,
                        routes=[("first", "fp32", "fp32"), TN]),
    "e-dx-fp32":   dict(hidden=[128, 64], out=32, B=2, N=48, precision="fp32", min_rows=1, want_dx=True,
                        routes=[FP32, FP32, FP32]),
    # (f) packed
    "f-packed":    dict(hidden=[256, 512], out=64, counts=[700, 1, 579], precision="bf16x3", min_rows=1, routes=[FIRST, TN, TR]),
    "f-cap-host":  dict(hidden=[256, 512], out=64, counts=[700, 1, 579], capacity=1536, precision="bf16x3", min_rows=1,
                        routes=[FIRST, TN, TR]),
    "f-cap-dev":   dict(hidden=[256, 512], out=64, counts=[700, 1, 579], capacity=1536, on_dev=True, precision="bf16x3",
                        min_rows=1, routes=[FIRST, TN, TR]),
    # (g) one bf16 product per element, production selection (1280 rows >= SPLIT_MIN_ROWS)
    "g-bf16":      dict(hidden=[256, 512], out=64, B=2, N=640, precision="bf16", min_rows=None, routes=[FIRST, TN, TR]),
}


@contextlib.contextmanager
def mode(precision, min_rows):
    from wf3d import config
    old = (config.precision(), config.SPLIT_MIN_ROWS)
    config.set_precision(precision)
    if min_rows is not None:
        config.SPLIT_MIN_ROWS = min_rows
    try:
        yield
    finally:
        config.set_precision(old[0])
        config.SPLIT_MIN_ROWS = old[1]


_ENCODERS = {}


def encoder(cfg, ps=None):
    from models.PointNetEncoder import PointNetEncoder
    key = (cfg.get("din", 8), tuple(cfg["hidden"]), cfg["out"])
    if key not in _ENCODERS:
        torch.manual_seed(20)
        enc = PointNetEncoder(key[0], cfg["hidden"], cfg["out"]).to(dev())
        E.perturb_1d(enc)
        _ENCODERS[key] = enc
    enc = _ENCODERS[key]
    enc.zero_grad(set_to_none=True)
    ps = SITE_PS[:len(cfg["hidden"])] if ps is None else ps
    for i, p in enumerate(ps):
        enc.mlp[4 * i + 3].p = p
    enc.precision = None
    return enc.set_packed_tail("compute").train(), ps


def run_encoder(enc, cfg, x, tail="compute", requires_grad=False):
    """(outs, pf as returned, input leaf, rows the per-point MLP ran over, rows the clouds own)."""
    if "counts" not in cfg:
        xd = x.to(dev()).requires_grad_(requires_grad)
        g, pf, up = enc.encode(xd)
        return {"g": g, "pf": pf, "up": up}, pf, xd, x.shape[0] * x.shape[1], x.shape[0] * x.shape[1]
    counts, cap = cfg["counts"], cfg.get("capacity")
    M_ = sum(counts)
    pts = x
    if cap is not None:
        pts = torch.zeros(cap, x.shape[1])
        pts[:M_] = x
    enc.set_packed_tail(tail)
    arg = torch.tensor(counts, device=dev()) if cfg.get("on_dev") else counts
    g, pf, up = enc.encode_packed(pts.to(dev()), arg, capacity=cap)
    enc.set_packed_tail("compute")
    return {"g": g, "pf": pf[:M_], "up": up}, pf, None, cap or -(-M_ // 256) * 256, M_


class Result:
    pass


def drive(cid, tail="compute", tseed=None):
    """Case `cid` on the first borderline-free input (or on input / torch seed `tseed`): forward in train mode, the drawn
    seed read from the module, backward of all three cotangents, and the fp64 model under the same masks and the
    kernels' own decisions."""
    from oracle.frozen import capture_encoder_decisions
    from wf3d.functional import Route
    cfg = CASES[cid]
    din, want_dx = cfg.get("din", 8), cfg.get("want_dx", False)
    x3 = cfg["precision"] != "fp32"
    res = Result()
    with mode(cfg["precision"], cfg["min_rows"]):
        enc, ps = encoder(cfg)
        for seed in ([tseed] if tseed is not None else range(100, 100 + DRAWS)):
            x = E.packed_input(seed, cfg["counts"], din) if "counts" in cfg else E.dense_input(seed, cfg["B"], cfg["N"], din)
            torch.manual_seed(seed)
            enc.last_dropout_seed = None
            outs, pf_full, xd, rows, M_ = run_encoder(enc, cfg, x, tail, want_dx)
            frozen, n_border, node = capture_encoder_decisions(outs["g"], enc, kernel_masks=x3, rows=M_ if "counts" in cfg else None)
            if n_border == 0 or tseed is not None:
                break
        else:
            pytest.fail(f"no borderline-free input found in {DRAWS} draws")
        res.seed, res.routes, res.live, res.dseed = seed, list(node.routes), node.live, enc.last_dropout_seed
        assert res.routes == [Route(*r) for r in cfg["routes"]], (cid, res.routes)
        assert node.saved[0].shape[0] == rows and isinstance(res.dseed, int)
        # the seed is the first value torch's CPU generator gives after manual_seed: the module's one draw
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(seed)
            assert res.dseed == int(torch.empty((), dtype=torch.int64).random_().item())

        cot = E.cotangents(seed + 1000, {k: tuple(outs[k].shape) for k in E.OUTS})
        heads = {"g": outs["g"], "pf": pf_full, "up": outs["up"]}
        cots = {k: cot[k].to(dev()) for k in E.OUTS}
        if pf_full.shape[0] != outs["pf"].shape[0]:
            full = torch.zeros(tuple(pf_full.shape))
            full[:M_] = cot["pf"]
            cots["pf"] = full.to(dev())
        torch.autograd.backward([heads[k] for k in E.OUTS], [cots[k] for k in E.OUTS])
        res.got = E.np_grads(enc)
        res.outs = {k: v.detach().clone() for k, v in outs.items()}

        P = E.params64(enc)
        widths = cfg["hidden"]
        masks = M.encoder_masks(res.dseed, ps, M_, widths)            # row = the buffer row: the clouds' rows come first
        assert sorted(masks) == sorted(M.encoder_sites(len(widths)))
        x64 = x.double().requires_grad_(want_dx)
        if "counts" in cfg:
            ref = M.ref_packed(P, x64, cfg["counts"], masks, frozen)
        else:
            ref = M.ref_dense(P, x64, masks, frozen)
        ref = dict(zip(E.OUTS, ref))
        sum((ref[k] * cot[k].double()).sum() for k in E.OUTS).backward()
        res.fwd = E.out_errors(outs, ref)
        res.errs = E.grad_errors(res.got, P)
        if want_dx:
            res.errs["x"] = H.elem_err(xd.grad.cpu().numpy(), x64.grad.numpy())
        # the masks matter: without them the model is far from what the kernels computed
        with torch.no_grad():
            plain = M.ref_packed(P, x64, cfg["counts"], None, frozen) if "counts" in cfg else M.ref_dense(P, x64, None, frozen)
        res.plain = H.rel_err(outs["pf"].detach().cpu().numpy(), plain[1].numpy())
    if cfg["precision"] == "bf16":
        from test_precision_bf16_gpu import TOL_BF16_FWD, TOL_BF16_GRAD
        res.tol_fwd, res.tol = TOL_BF16_FWD, TOL_BF16_GRAD
    else:
        res.tol_fwd, res.tol = TOL, cfg.get("tol", TOL_X3_FORCED if x3 else TOL)
    return res


def check(res, tag):
    worst = sorted(((e, n) for n, e in res.errs.items()), reverse=True)[:3]
    print(f"{tag} (seed {res.seed}): worst gradient errors {[(f'{e:.1e}', n) for e, n in worst]} (bound {res.tol:.1e}); forward "
          f"{ {k: (f'{a:.1e}', f'{b:.1e}') for k, (a, b) in res.fwd.items()} } (bound {res.tol_fwd:.1e}); without the masks "
          f"point_features would be {res.plain:.1e} off")
    for k, (a, b) in res.fwd.items():
        assert a < res.tol_fwd and b < res.tol_fwd, (tag, k, a, b)
    bad = [(n, e) for n, e in res.errs.items() if not e <= res.tol]
    assert not bad, (tag, res.seed, bad)
    assert res.plain > 1e-2, res.plain


@pytest.mark.parametrize("cid", [c for c in CASES])
def test_encoder_train_mode_vs_fp64_model_with_replayed_masks(cid):
    res = drive(cid)
    check(res, cid)
    cfg = CASES[cid]
    assert len(res.errs) == 4 * len(cfg["hidden"]) + 2 + 10 + (1 if cfg.get("want_dx") else 0)
    assert res.live is None


def test_routes_covered():
    """The cases' asserted routes cover every kernel family a site's mask goes through."""
    fwd, wgrad, dgrad = set(), set(), set()
    for cfg in CASES.values():
        for f, w, d in cfg["routes"]:
            fwd.add(f), wgrad.add(w), dgrad.add(d)
    assert fwd == {"first", "split", "fp32"}
    assert wgrad == {"first", "tn", "transposes", "fp32"}
    assert dgrad >= {"split", "fp32"}


def test_packed_tail_skip_is_bit_equal_to_compute_under_the_same_seed():
    """capacity 1536, 1280 live rows: "skip" stops at row 1280.  The mask is a function of (row, col) alone, so every
    output and gradient equals the "compute" run's bit for bit; and the run holds the model's bounds."""
    res = drive("f-cap-dev", tail="skip")
    assert res.live is not None, "the skip run fell back to computing the tail"
    check(res, "f-cap-dev skip")
    ref = drive("f-cap-dev", tail="compute", tseed=res.seed)
    assert ref.live is None and ref.dseed == res.dseed
    for k in ("g", "up"):
        assert torch.equal(ref.outs[k], res.outs[k]), k
    assert torch.equal(ref.outs["pf"], res.outs["pf"])
    for n, a in ref.got.items():
        assert torch.equal(a, res.got[n]), n


# ----------------------------------------------------------------------------------------------------------------------
# plumbing
# ----------------------------------------------------------------------------------------------------------------------
def _count_draws(monkeypatch):
    from wf3d.random import DropoutGenerator
    n = [0]
    orig = DropoutGenerator.draw

    def draw(self, out=None):
        n[0] += 1
        return orig(self, out)
    monkeypatch.setattr(DropoutGenerator, "draw", draw)
    return n


def test_eval_and_p0_draw_nothing_and_are_todays_bits(monkeypatch):
    cfg = CASES["a-tn"]
    with mode("bf16x3", 1):
        enc, _ = encoder(cfg, ps=(0.0, 0.0))
        x = E.dense_input(100, 2, 640).to(dev())
        want = [t.detach().clone() for t in enc.encode(x)]             # a module whose p was never raised
        enc, _ = encoder(cfg, ps=(0.5, 0.5))
        draws = _count_draws(monkeypatch)
        state = torch.get_rng_state()
        got = enc.eval().encode(x)
        assert torch.equal(torch.get_rng_state(), state) and draws[0] == 0
        for a, b in zip(got, want):
            assert torch.equal(a, b)
        # train mode with p > 0 draws one host value and changes the output
        got = enc.train().encode(x)
        assert not torch.equal(torch.get_rng_state(), state) and draws[0] == 0
        assert not torch.equal(got[1], want[1])
        # p = 0.5 against p = 0 in train mode: about half of point_features' inputs are gone
        assert H.rel_err(got[1].detach().cpu().numpy(), want[1].cpu().numpy()) > 1e-2
        encoder(cfg)


@pytest.mark.parametrize("site", [0, 1])
def test_p_one_is_refused_naming_the_site(site):
    cfg = CASES["a-tn"]
    ps = [0.1, 0.1]
    ps[site] = 1.0
    enc, _ = encoder(cfg, ps=tuple(ps))
    x = E.dense_input(100, 2, 64).to(dev())
    with pytest.raises(ValueError, match=rf"mlp\.{4 * site + 3}"):
        enc.encode(x)
    enc.eval().encode(x)                                                # eval mode does not look at p
    encoder(cfg)


def test_stream_setting_is_left_while_a_site_is_active():
    """WF3D_INFERENCE=stream under no_grad in train mode with an active site: the masked (non-stream) result, and the
    direct stream entry points refuse."""
    from wf3d import config
    cfg = CASES["a-tn"]
    with mode("bf16x3", 1):
        enc, _ = encoder(cfg, ps=(0.0, 0.3))
        x = E.dense_input(100, 2, 640).to(dev())
        old = config.inference()
        try:
            with torch.no_grad():
                torch.manual_seed(3)
                want = enc(x)
                config.set_inference("stream")
                torch.manual_seed(3)
                got = enc(x)
                with pytest.raises(ValueError, match="no dropout"):
                    enc.encode_stream(x)
                plain = enc.eval()(x)                                    # eval: the stream path serves it
        finally:
            config.set_inference(old)
        for a, b in zip(got, want):
            assert torch.equal(a, b)
        assert not torch.equal(got[1], plain[1])
        encoder(cfg)


def test_device_seed_words_serve_four_sites(monkeypatch):
    """dropout_rng "device": one draw per forward, site k masks with words[k] (checked against the fp64 model's forward);
    five hidden layers with an active fifth site raise, an inactive fifth does not; host mode takes any depth."""
    from models.PointNetEncoder import PointNetEncoder
    from wf3d import config
    old = config.dropout_rng()
    draws = _count_draws(monkeypatch)
    try:
        with mode("bf16x3", 1):
            config.set_dropout_rng("device")
            cfg = CASES["b-transposes"]
            enc, ps = encoder(cfg)
            x = E.dense_input(100, 2, 100)
            g, pf, up = enc.encode(x.to(dev()))
            assert draws[0] == 1
            words = enc.last_dropout_seeds.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
            assert list(words[1:]) == D.site_seeds(int(words[0]))
            masks = M.encoder_masks(None, ps, 200, cfg["hidden"], words=words)
            with torch.no_grad():
                ref = M.ref_dense(E.params64(enc), x.double(), masks)
            assert H.rel_err(pf.detach().cpu().numpy(), ref[1].numpy()) < 1e-3      # the right masks; decisions not frozen
            g.sum().backward()                                                       # the backward reads the same words
            encoder(cfg)
        with mode("bf16x3", None):
            torch.manual_seed(4)
            deep = PointNetEncoder(8, [32] * 5, 16).to(dev()).train()
            xs = E.dense_input(100, 2, 16).to(dev())
            deep.mlp[19].p = 0.2
            with pytest.raises(ValueError, match=r"mlp\.19"):
                deep.encode(xs)
            n = draws[0]
            deep.mlp[19].p, deep.mlp[3].p = 0.0, 0.2
            deep.encode(xs)[0].sum().backward()
            assert draws[0] == n + 1
            config.set_dropout_rng("host")
            deep.mlp[19].p = 0.2
            deep.encode(xs)[0].sum().backward()
            assert draws[0] == n + 1 and isinstance(deep.last_dropout_seed, int)
    finally:
        config.set_dropout_rng(old)
