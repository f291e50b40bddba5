"""Train-mode dropout of the HIP path against the host restatement of its masks (oracle/dropout.py) and the fp64 oracle.

Every dropout mask of the edge head is a pure function of (seed, row, column) (csrc/wf3d_common.h, wf3d_keep): the host
recomputes each bit, so the kernels are not only checked against each other with the same seed (tests/test_kernels_gpu.py)
but against an independent statement of WHICH element each mask drops:

a. every kernel that applies a mask, element by element: exactly 0 where the host drops, the undropped value times the
   fp32 scale 1/(1-p) elsewhere (forward kernels); backward kernels against the same kernel at p = 0 on a cotangent the
   host masked (the two runs do the same arithmetic on the same floats);
b. attention on its three paths (MFMA, VALU, VALU over key chunks) against fp64 torch math with the host mask on the
   softmax weights, at the no-dropout bounds;
c. the drop-in EdgePredictor in train mode, a different p at each of its four sites, against the oracle fed the masks
   of the seed the forward drew (oracle.reference_cpu, drop=; itself pinned to the reference's own train-mode run by
   tests/test_dropout_oracle.py), on every EdgeFn branch, every output and every parameter-gradient element;
d. the whole model at the production kernel selection in train mode, decision-frozen (tests/test_frozen_grad_gpu.py);
e. plumbing: eval mode and p = 0 draw nothing and launch no mask; p = 1 is refused with an error naming dropout.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import helpers as H  # noqa: E402
from helpers import oracle, unpack_sx8  # noqa: E402
from oracle import dropout as D  # noqa: E402

PS = (0.1, 0.5)
SEEDS = (0x2545F491, 0xDEADBEEF)                 # the second >= 2^31
SITE_PS = (0.05, 0.1, 0.2, 0.3)                  # vertex_proj.5, attention, edge_mlp.3, edge_mlp.7: all different
TOL_ELT = 2e-5


@pytest.fixture(scope="module")
def ops():
    from wf3d import ops as o
    o._lib.load()
    return o


def dev():
    return torch.device("cuda:0")


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed + 1000 * len(shape) + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).to(dev())


def host_keep(seed, R, C, p, row0=0):
    """[R, C] bool keep mask of rows row0 .. row0 + R - 1 (CPU)."""
    return torch.from_numpy(D.keep(seed, np.arange(row0, row0 + R)[:, None], np.arange(C)[None, :], p))


def scale32(p):
    return float(D.thresh_scale(p)[1])


def assert_masked_exact(got, undropped, keep, p):
    """Forward kernel output: exactly 0 where the host drops, exactly fl32(undropped * scale) where it keeps."""
    got, undropped = got.cpu(), undropped.cpu()
    assert got.shape == keep.shape
    want = torch.where(keep, undropped * scale32(p), torch.zeros_like(undropped))
    bad = got != want
    assert not bad.any(), (int(bad.sum()), "of", bad.numel(), "elements differ; first at", bad.nonzero()[:4].tolist())


def assert_masked_close(got, undropped, keep, p, tol):
    """Same for an sx8 output (hi + lo carries ~16 bits): zeros exact, kept values element-wise within tol."""
    got, undropped = got.cpu().double(), undropped.cpu().double()
    assert torch.equal(got[~keep], torch.zeros_like(got[~keep])), int((got[~keep] != 0).sum())
    want = torch.where(keep, undropped * scale32(p), torch.zeros_like(undropped))
    assert bool((got[keep & (undropped != 0)] != 0).all())          # nothing the host keeps is dropped
    e = H.elem_err(got.numpy(), want.numpy())
    assert e < tol, e


def ln_stats(ops, R, D_, seed):
    Z = rnd(R, D_, seed=seed, scale=1.5) + 0.2
    gamma, beta = 1 + 0.2 * rnd(D_, seed=seed + 1), 0.1 * rnd(D_, seed=seed + 2)
    mu, rs = ops.row_stats(Z)
    return Z, gamma, beta, mu, rs


# ---------------------------------------------------------------------------
# a. every kernel that applies a mask, against the host mask
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("act", [0, 2])
def test_ln_act_apply_mask_is_the_host_mask(ops, p, seed, act):
    R, D_ = 2500, 512                                # 1.28 M elements: many workgroups, grid-stride rows far from 0
    Z, gamma, beta, mu, rs = ln_stats(ops, R, D_, 1)
    got = ops.ln_act_apply(Z, mu, rs, gamma, beta, act, drop_p=p, seed=seed)
    ref = ops.ln_act_apply(Z, mu, rs, gamma, beta, act)
    assert_masked_exact(got, ref, host_keep(seed, R, D_, p), p)


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("x3", [False, True])
def test_gemm_prologue_mask_is_the_host_mask_nt_and_tn(ops, p, seed, x3):
    """The GEMM prologue drop(act(LN(z))) on the A operand (NT, forward) and on the B operand (TN, wgrad); 700 rows =
    several 256-row tiles with a ragged last one.  fp64 product of the host-masked activation."""
    M, K, N = 700, 512, 200
    Z, gamma, beta, mu, rs = ln_stats(ops, M, K, 3)
    W = rnd(N, K, seed=6)
    pro = ops.Pro(ops.ACT_GELU, mu, rs, gamma, beta, p, seed)
    h = ops.ln_act_apply(Z, mu, rs, gamma, beta, ops.ACT_GELU).double().cpu()
    hd = h * host_keep(seed, M, K, p).double() * scale32(p)
    tol = 1e-4
    got = ops.gemm(Z, W, ops.NT, pro=pro, x3=x3)
    assert H.rel_err(got.cpu().numpy(), (hd @ W.double().cpu().T).numpy()) < tol
    G = rnd(M, N, seed=7)
    got = ops.gemm(G, Z, ops.TN, pro=pro, x3=x3)
    assert H.rel_err(got.cpu().numpy(), (G.double().cpu().T @ hd).numpy()) < tol


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("seed", SEEDS)
def test_ln_prep_mask_is_the_host_mask(ops, p, seed):
    R, D_ = 1500, 512
    Z, gamma, beta, _, _ = ln_stats(ops, R, D_, 4)
    mu, rs, hs = ops.ln_prep(Z, gamma, beta, ops.ACT_GELU, drop_p=p, seed=seed)
    hi, lo = unpack_sx8(hs)
    ref = ops.ln_act_apply(Z, mu, rs, gamma, beta, ops.ACT_GELU)
    assert_masked_close(hi + lo, ref, host_keep(seed, R, D_, p), p, 3e-5)


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("seed", SEEDS)
def test_split_transpose_prologue_mask_is_the_host_mask(ops, p, seed):
    """sx8 [C, R] = split(drop(act(LN(z)))^T): the mask is indexed by the row of z, not by the transposed tile."""
    R, C = 1000, 512
    Z, gamma, beta, mu, rs = ln_stats(ops, R, C, 5)
    hi, lo = unpack_sx8(ops.split_transpose(Z, ops.Pro(ops.ACT_GELU, mu, rs, gamma, beta, p, seed)))
    ref = ops.ln_act_apply(Z, mu, rs, gamma, beta, ops.ACT_GELU)
    assert_masked_close((hi + lo).T.contiguous(), ref, host_keep(seed, R, C, p), p, 3e-5)


def _pair_inputs(ops, H_, counts):
    meta = ops.EdgeMeta(counts, dev())
    Pa, Pb = rnd(meta.Rv, H_, seed=11), rnd(meta.Rv, H_, seed=12)
    cv = rnd(meta.Rv, 3, seed=13)
    W0 = rnd(H_, 2 * H_ + 7, seed=14, scale=0.2)
    gamma, beta = 1.0 + 0.1 * rnd(H_, seed=15), 0.1 * rnd(H_, seed=16)
    return meta, Pa, Pb, cv, W0, gamma, beta


PAIR_COUNTS = [40, 2, 17, 33, 64]                # 3,461 edge rows over five samples: rows are eoff[s] + e


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("keep_pre", [True, False])
def test_edge_pair_fwd_ln_mask_is_the_host_mask(ops, p, seed, keep_pre):
    H_ = 512
    meta, Pa, Pb, cv, W0, gamma, beta = _pair_inputs(ops, H_, PAIR_COUNTS)
    pre, mu, rs, delta = ops.edge_pair_fwd(Pa, Pb, cv, W0, meta)
    _, mu2, rs2, _, h = ops.edge_pair_fwd(Pa, Pb, cv, W0, meta, ln=(gamma, beta, ops.ACT_GELU, p, seed), keep_pre=keep_pre)
    hi, lo = unpack_sx8(h)
    ref = ops.ln_act_apply(pre, mu2, rs2, gamma, beta, ops.ACT_GELU)
    assert_masked_close(hi + lo, ref, host_keep(seed, meta.Re, H_, p), p, 3e-5)


def _bwd_pair(run, dh, keep, p):
    """(kernel with the mask, same kernel at p = 0 on the host-masked cotangent)."""
    dhm = dh * keep.to(dh.device) * scale32(p)
    return run(dh.clone(), p), run(dhm, 0.0)


def _close(a, b, tol=1e-6, floor=None):
    if a is None or b is None:
        assert a is None and b is None
        return
    e = H.elem_err(a.cpu().numpy(), b.cpu().numpy(), floor)
    assert e < tol, e


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("act", [0, 2])
def test_ln_act_bwd_mask_is_the_host_mask(ops, p, seed, act):
    """LayerNorm(+act) backward with the mask on the incoming gradient, in its three output forms: fp32 dz, fp32 + sx8
    dz (dz_split), sx8 only (want_dz=False).  A single misplaced mask bit moves its own dz element by ~|dh| * rstd."""
    R, D_ = 1500, 512
    Z, gamma, beta, mu, rs = ln_stats(ops, R, D_, 6)
    dh = rnd(R, D_, seed=20)
    keep = host_keep(seed, R, D_, p)

    def plain(d, pp):
        return ops.ln_act_bwd(d, Z, mu, rs, gamma, beta, act, pp, seed)

    (dz, dg, db, dbias), (dz0, dg0, db0, dbias0) = _bwd_pair(plain, dh, keep, p)
    _close(dz, dz0); _close(dg, dg0); _close(db, db0); _close(dbias, dbias0)

    def split(d, pp):
        s = torch.zeros_like(Z)
        out = ops.ln_act_bwd(d, Z, mu, rs, gamma, beta, act, pp, seed, dz_split=s)
        return out[0], s

    (dz1, s1), (dz01, s01) = _bwd_pair(split, dh, keep, p)
    _close(dz1, dz0)
    hi, lo = unpack_sx8(s1)
    _close(hi + lo, dz0, 3e-5)

    def split_only(d, pp):
        s = torch.zeros_like(Z)
        out = ops.ln_act_bwd(d, Z, mu, rs, gamma, beta, act, pp, seed, dz_split=s, want_dz=False)
        assert out[0] is None
        return s

    s2, _ = _bwd_pair(split_only, dh, keep, p)
    assert torch.equal(s2, s1)


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("seed", SEEDS)
def test_ln_act_bwd_wsum_mask_is_the_host_mask(ops, p, seed):
    R, D_ = 1500, 512
    Z, gamma, beta, mu, rs = ln_stats(ops, R, D_, 7)
    wrow = rnd(R, seed=21).abs()
    dh = rnd(R, D_, seed=22)

    def run(d, pp):
        return ops.ln_act_bwd_wsum(d, Z, wrow, mu, rs, gamma, beta, ops.ACT_GELU, pp, seed)

    got, ref = _bwd_pair(run, dh, host_keep(seed, R, D_, p), p)
    for a, b in zip(got, ref):
        _close(a, b)


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("seed", SEEDS)
def test_edge_pair_ln_bwd_mask_is_the_host_mask(ops, p, seed):
    """The LayerNorm backward that rebuilds the first edge layer's row from Pa / Pb: mask on global edge rows."""
    H_ = 512
    meta, Pa, Pb, cv, W0, gamma, beta = _pair_inputs(ops, H_, PAIR_COUNTS)
    _, mu, rs, delta = ops.edge_pair_fwd(Pa, Pb, cv, W0, meta)
    dh = rnd(meta.Re, H_, seed=23)

    def run(d, pp):
        return ops.edge_pair_ln_bwd(d, Pa, Pb, delta, W0, meta, mu, rs, gamma, beta, ops.ACT_GELU, pp, seed)

    got, ref = _bwd_pair(run, dh, host_keep(seed, meta.Re, H_, p), p)
    for a, b in zip(got, ref):
        _close(a, b)


# ---------------------------------------------------------------------------
# b. attention, all three paths, against fp64 torch math with the host mask
# ---------------------------------------------------------------------------
def attn_ref(qkv64, counts, E, heads, p, seed):
    """ctx = ((softmax(S) * M) * scale) V per sample and head, M the host mask at rows (voff + i) * heads + h."""
    voff, _ = D.offsets(counts)
    hd = E // heads
    outs = []
    for s, c in enumerate(counts):
        blk = qkv64[voff[s]:voff[s] + c]
        q, k, v = blk[:, :E], blk[:, E:2 * E], blk[:, 2 * E:]
        sp = lambda t: t.reshape(c, heads, hd).transpose(0, 1)     # noqa: E731
        w = torch.softmax((sp(q) / hd ** 0.5) @ sp(k).transpose(-1, -2), -1)
        if p > 0:
            w = w * torch.from_numpy(D.attention_weights(voff[s], c, heads, seed, p))
        outs.append((w @ sp(v)).transpose(0, 1).reshape(c, E))
    return torch.cat(outs)


@pytest.mark.parametrize("E,heads,counts", [
    (512, 8, [5, 64, 130, 256, 2]),              # head_dim 64, vmax <= 256: MFMA kernels (the production edge head)
    (128, 4, [5, 64, 130, 256, 2]),              # head_dim 32: VALU kernels
    (128, 4, [300, 513, 7, 257]),                # VALU over key chunks (vmax > 256)
    (512, 8, [300, 7, 257]),                     # head_dim 64 beyond 256 keys: VALU chunked too
])
@pytest.mark.parametrize("p,seed", [(0.1, 0xDEADBEEF), (0.5, 0x2545F491)])
def test_attention_dropout_vs_fp64_with_host_mask(ops, E, heads, counts, p, seed):
    torch.manual_seed(2)
    meta = ops.EdgeMeta.get(counts, dev())
    qkv = torch.randn(meta.Rv, 3 * E, device=dev())
    dctx = torch.randn(meta.Rv, E, device=dev())
    ctx, lse = ops.attn_fwd(qkv, meta, E, heads, p, seed)
    dqkv = ops.attn_bwd(qkv, dctx, ctx, lse, meta, E, heads, p, seed)
    q64 = qkv.double().cpu().requires_grad_()
    ref = attn_ref(q64, counts, E, heads, p, seed)
    e_ctx = H.rel_err(ctx.cpu().numpy(), ref.detach().numpy())
    (ref * dctx.double().cpu()).sum().backward()
    e_d = H.rel_err(dqkv.cpu().numpy(), q64.grad.numpy())
    print(f"attention E={E} heads={heads} vmax={max(counts)} p={p}: ctx {e_ctx:.2e} (< 2e-5), dqkv {e_d:.2e} (< 1e-4)")
    assert e_ctx < 2e-5
    assert e_d < 1e-4
    # the undropped lse: dropout acts after the softmax normaliser
    ctx0, lse0 = ops.attn_fwd(qkv, meta, E, heads)
    assert torch.equal(lse, lse0)


# ---------------------------------------------------------------------------
# c. the edge head in train mode against the dropout-aware oracle
# ---------------------------------------------------------------------------
SPIED = ("edge_pair_fwd", "ln_prep", "split_transpose", "gemm", "gemm_split_tn", "edge_pair_ln_bwd", "ln_act_bwd_wsum",
         "rowdot_act_bwd", "ln_act_apply", "attn_fwd", "attn_bwd", "ln_act_bwd")


@pytest.fixture
def spy(monkeypatch):
    """Records the wf3d.ops calls EdgeFn makes (name, args, kwargs), to assert which branch ran."""
    from wf3d import ops
    calls = []
    for n in SPIED:
        orig = getattr(ops, n)

        def w(*a, _n=n, _o=orig, **k):
            calls.append((_n, a, k))
            return _o(*a, **k)
        monkeypatch.setattr(ops, n, w)
    return calls


def _pro_of(name, a, k):
    if name == "gemm":
        return k.get("pro"), a[2]
    if name == "split_transpose":
        return (a[1] if len(a) > 1 else k.get("pro")), None
    return None, None


def branches(calls):
    """What the spied calls say about the EdgeFn branches that ran."""
    b = {"pair_ln": [], "keep_pre": [], "prep_drop": [], "st_drop": [], "gemm_nt_drop": [], "gemm_tn_drop": [],
         "tn": 0, "pair_ln_bwd": 0, "wsum": 0, "rowdot_bwd": 0}
    for n, a, k in calls:
        if n == "edge_pair_fwd" and k.get("ln") is not None:
            b["pair_ln"].append(k["ln"][3])
            b["keep_pre"].append(k.get("keep_pre", True))
        elif n == "ln_prep":
            b["prep_drop"].append(k.get("drop_p", 0.0))
        elif n in ("split_transpose", "gemm"):
            pro, layout = _pro_of(n, a, k)
            if pro is not None and pro.drop_p > 0:
                key = "st_drop" if n == "split_transpose" else ("gemm_tn_drop" if layout == 2 else "gemm_nt_drop")
                b[key].append(round(pro.drop_p, 6))
        elif n == "gemm_split_tn":
            b["tn"] += 1
        elif n == "edge_pair_ln_bwd":
            b["pair_ln_bwd"] += 1
        elif n == "ln_act_bwd_wsum":
            b["wsum"] += 1
        elif n == "rowdot_act_bwd":
            b["rowdot_bwd"] += 1
    return b


def drop_seed_after(s):
    """The seed EdgePredictor.forward_ragged draws right after torch.manual_seed(s)."""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(s)
        return int(torch.empty((), dtype=torch.int64).random_().item())


def _set_site_ps(ep, ps):
    ep.vertex_proj[5].p, ep.attention.dropout, ep.edge_mlp[3].p, ep.edge_mlp[7].p = ps
    return ep


def edge_head_case(counts, precision, min_rows, hidden=512, heads=8, ps=SITE_PS, tseed=77):
    """Train-mode forward_ragged + backward against the oracle under the replayed masks.  Returns (errors, tol)."""
    from wf3d import config
    from models.EdgePredictor import EdgePredictor
    old = (config.precision(), config.SPLIT_MIN_ROWS)
    config.set_precision(precision)
    if min_rows is not None:
        config.SPLIT_MIN_ROWS = min_rows
    try:
        torch.manual_seed(5)
        ep = _set_site_ps(EdgePredictor(3, hidden, heads), ps).to(dev()).train()
        with torch.no_grad():
            for n, p_ in ep.named_parameters():
                if p_.dim() == 1:
                    p_.add_(0.05 * torch.randn(p_.shape, generator=torch.Generator().manual_seed(len(n))).to(dev()))
        g = torch.Generator().manual_seed(7)
        v = torch.randn(len(counts), max(counts), 3, generator=g)
        vg = v.clone().to(dev()).requires_grad_()
        torch.manual_seed(tseed)
        probs = ep.forward_ragged(vg, counts)
        seed = drop_seed_after(tseed)
        cot = torch.randn(probs.shape, generator=g)
        (probs * cot.to(dev())).sum().backward()
        torch.cuda.synchronize()
        masks = D.edge_head_masks(seed, counts, ps, hidden, heads)
        P = {"edge_predictor." + n: p_.detach().cpu().double().requires_grad_() for n, p_ in ep.named_parameters()}
        vr = v.double().requires_grad_()
        errs, tot = {}, 0.0
        e_out = 0.0
        for s, c in enumerate(counts):
            pr, _ = oracle.edge_forward(P, vr[s:s + 1, :c], num_heads=heads, drop=masks[s])
            e_out = max(e_out, H.elem_err(probs[s, :pr.shape[1]].detach().cpu().numpy(), pr[0].detach().numpy(), 1e-6))
            if pr.shape[1] < probs.shape[1]:
                assert float(probs[s, pr.shape[1]:].abs().max()) == 0.0          # padding exactly 0
            tot = tot + (pr[0] * cot[s, :pr.shape[1]].double()).sum()
        tot.backward()
        errs["<probs>"] = e_out
        errs["<vertices>"] = H.elem_err(vg.grad.cpu().numpy(), vr.grad.numpy())
        for n, p_ in ep.named_parameters():
            ref = P["edge_predictor." + n].grad
            if ref is None:
                assert p_.grad is None, n
                continue
            errs[n] = H.elem_err(p_.grad.cpu().numpy(), ref.numpy())
        return errs
    finally:
        config.set_precision(old[0])
        config.SPLIT_MIN_ROWS = old[1]


def _report(tag, errs, tol):
    worst = sorted(((e, n) for n, e in errs.items()), reverse=True)
    print(f"{tag}: worst element-wise errors (bound {tol:.0e})", [(f"{e:.2e}", n) for e, n in worst[:4]])
    assert errs["<probs>"] < 1e-4, errs["<probs>"]
    bad = [(n, e) for n, e in errs.items() if not e < tol]
    assert not bad, bad


P1, P2 = SITE_PS[2], SITE_PS[3]


def test_edge_head_train_mode_fp32_unsplit_path(spy):
    """fp32: the edge MLP on the fp32 GEMMs, both dropouts in their prologues (forward NT, wgrad TN)."""
    errs = edge_head_case([9, 2, 5, 12], "fp32", 1)
    b = branches(spy)
    assert b["pair_ln"] == [] and b["tn"] == 0 and b["st_drop"] == []
    assert sorted(set(b["gemm_nt_drop"])) == [P1, P2] and sorted(set(b["gemm_tn_drop"])) == [P1, P2]
    assert b["wsum"] == 1 and b["rowdot_bwd"] == 1
    _report("fp32 unsplit", errs, 1e-4)


@pytest.mark.parametrize("counts,wide,route", [
    ([9, 2, 5, 12], False, "gemm"),             # 113 edge rows (odd): split forward, wgrads on the fp32-operand TN GEMM
    ([16, 9, 8], False, "transpose"),           # 184 rows: whole 8-row groups, not 32: wgrads through split_transpose
    ([12, 12, 8], False, "tn"),                 # 160 rows: transposing-read TN kernel, pre not stored (rebuilt)
    ([12, 12, 8], True, "tn"),                  # same at hidden 2048: pre stored (edge_pair_ln_bwd takes H <= 1024)
])
def test_edge_head_train_mode_split_paths(spy, counts, wide, route):
    """bf16x3 forced onto the split path (SPLIT_MIN_ROWS = 1) at edge-row counts that select each wgrad route; bound as
    the p = 0 forced cases (tests/test_model_gpu.py::test_edge_head_other_hidden_sizes_vs_oracle: 3e-4)."""
    errs = edge_head_case(counts, "bf16x3", 1, hidden=2048 if wide else 512)
    b = branches(spy)
    assert b["pair_ln"] == [P1] and b["prep_drop"] == [P2] and b["rowdot_bwd"] == 1
    if route == "gemm":
        assert b["tn"] == 0 and b["st_drop"] == [] and sorted(set(b["gemm_tn_drop"])) == [P1, P2]
    elif route == "transpose":
        assert b["tn"] == 0 and sorted(b["st_drop"]) == [P1, P2] and b["gemm_tn_drop"] == []
    else:
        assert b["tn"] == 2 and b["st_drop"] == [] and b["gemm_tn_drop"] == []
    want_keep = wide or route != "tn"
    assert b["keep_pre"] == [want_keep]
    assert (b["wsum"], b["pair_ln_bwd"]) == ((1, 0) if want_keep else (0, 1))
    _report(f"bf16x3 forced, {route}, keep_pre={want_keep}", errs, 3e-4)


def test_edge_head_train_mode_valu_attention():
    """hidden 256 / 8 heads: head_dim 32, the VALU attention kernels inside the edge head."""
    errs = edge_head_case([9, 2, 6], "fp32", 1, hidden=256, heads=8)
    _report("fp32 VALU attention", errs, 1e-4)


def test_edge_head_train_mode_at_the_bench_shape(spy):
    """cfg2's edge head (B = 32, V = 64: 64,512 edge rows) at the production kernel selection in bf16x3 mode; bound as
    the p = 0 production-selection tests (2e-4)."""
    errs = edge_head_case([64] * 32, "bf16x3", None)
    b = branches(spy)
    assert b["pair_ln"] == [P1] and b["prep_drop"] == [P2] and b["tn"] == 2 and b["keep_pre"] == [False]
    _report("cfg2 edge head, production selection", errs, 2e-4)


# ---------------------------------------------------------------------------
# d. the whole model at the production kernel selection, train mode, decision-frozen
# ---------------------------------------------------------------------------
def test_frozen_gradients_production_kernel_selection_train_mode():
    """As tests/test_frozen_grad_gpu.py::test_frozen_gradients_production_kernel_selection with the reference's p = 0.1 at
    all four edge-head sites; the oracle replays the masks of the seed the forward drew."""
    from test_frozen_grad_gpu import TOL, TOL_X3, _run
    counts = [64, 33, 2, 7, 50, 64, 12, 40]
    fwd, errs, seed = _run("bf16x3", 8, 4096, 64, counts, min_rows=None, kernel_masks=True, draws=8, drop_p=0.1)
    worst = sorted(((e, n) for n, e in errs.items()), reverse=True)
    print(f"train mode, bf16x3 production selection (input seed {seed}): worst", [(f"{e:.2e}", n) for e, n in worst[:5]])
    for k, (a, b) in fwd.items():
        assert a < TOL and b < TOL, (k, a, b)
    assert len(errs) == 76
    bad = [(n, e) for n, e in errs.items() if not e <= TOL_X3]
    assert not bad, bad


def test_bf16_frozen_gradients_production_kernel_selection_train_mode():
    from test_frozen_grad_gpu import _run
    from test_precision_bf16_gpu import TOL_BF16_FWD, TOL_BF16_GRAD
    counts = [64, 33, 2, 7, 50, 64, 12, 40]
    fwd, errs, seed = _run("bf16", 8, 4096, 64, counts, min_rows=None, kernel_masks=True, draws=8, drop_p=0.1)
    worst = sorted(((e, n) for n, e in errs.items()), reverse=True)
    print(f"train mode, bf16 production selection (input seed {seed}): worst", [(f"{e:.2e}", n) for e, n in worst[:3]])
    for k, (a, b) in fwd.items():
        assert a < TOL_BF16_FWD and b < TOL_BF16_FWD, (k, a, b)
    bad = [(n, e) for n, e in errs.items() if not e <= TOL_BF16_GRAD]
    assert not bad, bad


# ---------------------------------------------------------------------------
# e. plumbing
# ---------------------------------------------------------------------------
def test_eval_mode_and_p0_draw_nothing_and_match_bit_for_bit(spy):
    """p = 0 in train mode and any p in eval mode: no seed is drawn from torch's generator, no kernel gets a mask, and
    the output is bit-identical to the p = 0 path."""
    from models.EdgePredictor import EdgePredictor
    torch.manual_seed(5)
    ep = EdgePredictor(3, 512, 8).to(dev())
    v = torch.randn(3, 12, 3, generator=torch.Generator().manual_seed(3)).to(dev())
    counts = [12, 5, 9]
    _set_site_ps(ep, (0.0, 0.0, 0.0, 0.0)).train()
    st = torch.get_rng_state()
    with torch.no_grad():
        a = ep.forward_ragged(v, counts)
    assert torch.equal(st, torch.get_rng_state())
    _set_site_ps(ep, SITE_PS).eval()
    with torch.no_grad():
        b = ep.forward_ragged(v, counts)
    assert torch.equal(st, torch.get_rng_state())
    assert torch.equal(a, b)
    for n, a_, k in spy:
        assert k.get("drop_p", 0.0) == 0.0, n
        if n == "edge_pair_fwd" and k.get("ln") is not None:
            assert k["ln"][3] == 0.0
        if n == "attn_fwd":
            assert a_[4] == 0.0
        pro, _ = _pro_of(n, a_, k)
        assert pro is None or pro.drop_p == 0.0, n
    # and train mode with p > 0 does draw one seed, and changes the output
    ep.train()
    with torch.no_grad():
        c = ep.forward_ragged(v, counts)
    assert not torch.equal(st, torch.get_rng_state()) and not torch.equal(a, c)


@pytest.mark.parametrize("site", range(4))
def test_p_one_is_refused_naming_dropout(site):
    """torch allows p = 1 (the site's output is all zeros); the HIP edge head refuses it with a clear error instead of
    launching (the kernels take p in [0, 1)).  Eval mode ignores p, so p = 1 there runs."""
    from models.EdgePredictor import EdgePredictor
    torch.manual_seed(5)
    ps = list(SITE_PS)
    ps[site] = 1.0
    ep = _set_site_ps(EdgePredictor(3, 64, 2), ps).to(dev()).train()
    v = torch.randn(2, 5, 3, device=dev())
    with pytest.raises(ValueError, match="dropout"):
        ep.forward_ragged(v, [5, 3])
    ep.eval()
    with torch.no_grad():
        assert torch.isfinite(ep.forward_ragged(v, [5, 3])).all()
