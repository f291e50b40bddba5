"""Kernels on inputs that no Gaussian draw supplies (every input here is finite).

A. coincident vertices: |c_i - c_j| = 0 exactly.  The distance term of the pair backward then contributes exactly zero
   (torch's rule for the norm at 0, which the fp64 oracle follows): the whole edge head in both precision modes, ragged
   and padded, on the stored and the rebuilt first-pair-layer route, and ops.edge_pair_fwd / edge_pair_bwd directly.
B. attention logits in the tens (q scaled by 8 and 40) and a common shift of every key: VALU, resident MFMA, key-tiled.
C. LayerNorm rows whose mean is 1e2 / 1e3 times their spread: row_stats, ln_act_apply, ln_prep, ln_act_bwd, the fused
   first layer, the pair kernel's statistics, the skinny kernels' merged partial statistics.
D. probabilities at exactly 0 and 1 (and next to them) in WireframeLoss, and the small edge-head / vertex-head kernels
   (vertex_finalize, edge_prob, gather / scatter) called directly at saturating logits.

Bounds.  Where a kernel has a bound in its own test file that bound is the floor (tests/test_kernels_gpu.py,
tests/test_skinny_gpu.py, the attention bounds 2e-5 / 1e-4 / 1e-5).  The inputs of B and C (and the H = 2048 rows of A)
are worse conditioned in fp32 than Gaussian ones, so each test evaluates the same formula with plain fp32 torch on the
CPU, takes that evaluation's error against the fp64 reference, and allows the kernel max(4 x that error, floor): the
factor 4 covers another summation order.  The yardstick is torch, never the kernel.  Each test prints what it measured
and the bound it used."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import helpers as H  # noqa: E402
from helpers import oracle  # noqa: E402,F401

TOL_ELT = 2e-5          # tests/test_kernels_gpu.py: elementwise / reduction kernels
EPS = 1e-5


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from wf3d import ops as o
    o._lib.load()
    return o


@pytest.fixture(params=["fp32", "bf16x3"])
def precision(request):
    """Both arithmetic modes; bf16x3 is forced onto small shapes too (as tests/test_model_gpu.py)."""
    from wf3d import config
    old = (config.precision(), config.SPLIT_MIN_ROWS)
    config.set_precision(request.param)
    config.SPLIT_MIN_ROWS = 1
    yield request.param
    config.set_precision(old[0])
    config.SPLIT_MIN_ROWS = old[1]


def c64(t):
    return t.detach().double().cpu()


def scaled(a, b):
    """max|a - b| / max|b|: error on the tensor's scale (tests/test_kernels_gpu.py::rel)."""
    a, b = c64(a), c64(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    if a.numel() == 0:
        return 0.0
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def elementwise(a, b, floor):
    """max_i |a_i - b_i| / max(|b_i|, floor)."""
    a, b = c64(a), c64(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    if a.numel() == 0:
        return 0.0
    return float(((a - b).abs() / b.abs().clamp_min(floor)).max())


def held(tag, got, yard, floor):
    """Assert got <= max(4 * yard, floor), yard being fp32 torch's own error against the same fp64 reference."""
    bound = max(4.0 * yard, floor)
    print(f"{tag}: kernel {got:.2e}, fp32 torch {yard:.2e}, bound {bound:.2e}")
    assert got <= bound, (tag, got, yard, bound)


# ---------------------------------------------------------------------------
# A. coincident vertices
# ---------------------------------------------------------------------------
def _planted(counts, vd, seed, plant):
    """[B, max(counts), vd] vertices; plant: in every sample with >= 2 vertices two of them are the same point."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(len(counts), max(counts), vd, generator=g)
    if plant:
        for s, c in enumerate(counts):
            if c >= 2:
                v[s, min(4, c - 1)] = v[s, min(1, c - 2)]
    return v


def _degenerate_vertices(counts):
    """Sample 0: vertices 1 and 4 identical; sample 1: every vertex at the origin; the others Gaussian."""
    v = torch.randn(len(counts), max(counts), 3, generator=torch.Generator().manual_seed(21))
    v[0, 4] = v[0, 1]
    v[1] = 0.0
    return v


def _padded(tail):
    def run(ep, vg, counts):
        return ep.forward_padded(vg, torch.tensor(counts, device=dev()), tail=tail)
    return run


@pytest.mark.parametrize("layout", ["ragged", "padded-compute", "padded-skip"])
def test_edge_head_with_coincident_vertices_vs_oracle(layout, precision):
    """EdgePredictor(3, 64, 2), counts [6, 4]: vertices 1 and 4 of sample 0 identical, all four of sample 1 zero.  Forward
    and every gradient element against the fp64 oracle, bounds of tests/test_model_gpu.py::_edge_head_case (its pre-
    activation is stored at this size, in both modes)."""
    from test_model_gpu import _edge_head_case
    counts = [6, 4]
    run = None if layout == "ragged" else _padded(layout.split("-")[1])
    _edge_head_case(3, 64, 2, counts, precision, 91, vertices=_degenerate_vertices(counts), run=run)


@pytest.mark.parametrize("layout,counts", [("ragged", [12, 12, 8]), ("padded-compute", [12, 12, 8, 5]),
                                           ("padded-skip", [12, 12, 8, 5])])
def test_edge_head_with_coincident_vertices_rebuilt_preactivation(layout, counts, monkeypatch):
    """The same on the route that does not store the first pair layer's pre-activation (ops.edge_pair_ln_bwd rebuilds it
    from Pa / Pb and the stored delta = 0): bf16x3 forced, hidden 512, an edge-row total that is a multiple of 32 (160
    ragged as tests/test_dropout_gpu.py selects it; 4 x 120 padded to 16 vertices), bound 3e-4 of the forced cases."""
    from test_model_gpu import _edge_head_case
    from wf3d import config, ops as o
    calls = []
    orig = o.edge_pair_ln_bwd
    monkeypatch.setattr(o, "edge_pair_ln_bwd", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    old = (config.precision(), config.SPLIT_MIN_ROWS)
    config.set_precision("bf16x3")
    config.SPLIT_MIN_ROWS = 1
    try:
        run = None
        if layout != "ragged":
            # the layout is 16 vertices wide (4 x 120 edge rows); the helper sees the columns of the widest sample
            width = max(counts) * (max(counts) - 1) // 2
            padded = _padded(layout.split("-")[1])
            run = lambda ep, vg, c: padded(ep, torch.nn.functional.pad(vg, (0, 0, 0, 16 - vg.shape[1])), c)[:, :width]  # noqa: E731
        _edge_head_case(3, 512, 8, counts, "bf16x3", 92, vertices=_degenerate_vertices(counts), run=run)
    finally:
        config.set_precision(old[0])
        config.SPLIT_MIN_ROWS = old[1]
    assert calls == [1], "the rebuilt route did not run"


def _pair_index(counts):
    I, J, off = [], [], 0
    for c in counts:
        for i in range(c):
            for j in range(i + 1, c):
                I.append(off + i)
                J.append(off + j)
        off += c
    return torch.tensor(I, dtype=torch.long), torch.tensor(J, dtype=torch.long)


def _pair_math(Pa, Pb, cv, W0, I, J, dpre, dtype):
    """pre[e] = Pa[i] + Pb[j] + |c_i - c_j| w_delta in `dtype` on the CPU, its row statistics, and the gradients of
    sum(dpre * pre) without and with the coordinate columns c_i Wc^T + c_j Wd^T."""
    Hh, vd = Pa.shape[1], cv.shape[1]
    Pa, Pb, cv = (t.detach().cpu().to(dtype).requires_grad_() for t in (Pa, Pb, cv))
    W0, dpre = W0.detach().cpu().to(dtype), dpre.detach().cpu().to(dtype)
    delta = torch.linalg.vector_norm(cv[I] - cv[J], dim=-1)
    pre = Pa[I] + Pb[J] + delta[:, None] * W0[:, -1]
    mu = pre.mean(1)
    rs = 1.0 / torch.sqrt(pre.var(1, unbiased=False) + EPS)
    out = {"pre": pre.detach(), "mu": mu.detach(), "rs": rs.detach(), "delta": delta.detach()}
    gPa, gPb, gc = torch.autograd.grad((pre * dpre).sum(), (Pa, Pb, cv), retain_graph=True)
    out.update(dPa=gPa, dPb=gPb, dcv=gc)
    Wc, Wd = W0[:, 2 * Hh:2 * Hh + vd], W0[:, 2 * Hh + vd:2 * Hh + 2 * vd]
    full = pre + cv[I] @ Wc.T + cv[J] @ Wd.T
    out["dcv_coord"] = torch.autograd.grad((full * dpre).sum(), cv)[0]
    return out


PAIR_COUNTS = [[2] * 9 + [3], [5, 1, 0, 7], [40, 2, 17]]


@pytest.mark.parametrize("vd", [1, 3, 8])
@pytest.mark.parametrize("Hh", [64, 260, 1032, 2048])
def test_pair_kernels_vs_fp64(ops, Hh, vd):
    """ops.edge_pair_fwd and ops.edge_pair_bwd (coord=False / True) against fp64 autograd, at row widths of 1, 2 and 8
    column slices per lane (H = 2048: the widest instantiation), one edge per sample (a wave's 8 edge rows cross 8
    samples), samples without edges, and each layout once with random vertices and once with a coincident pair in
    every sample."""
    for counts in PAIR_COUNTS:
        meta = ops.EdgeMeta(counts, dev())
        I, J = _pair_index(counts)
        assert len(I) == meta.Re
        for plant in (False, True):
            g = torch.Generator().manual_seed(Hh + 10 * vd + len(counts))
            vs = _planted(counts, vd, Hh + vd, plant)
            cv = torch.cat([vs[s, :c] for s, c in enumerate(counts)]).contiguous().to(dev())
            Pa, Pb = (torch.randn(meta.Rv, Hh, generator=g).to(dev()) for _ in range(2))
            W0 = (0.2 * torch.randn(Hh, 2 * Hh + 2 * vd + 1, generator=g)).to(dev())
            dpre = torch.randn(meta.Re, Hh, generator=g).to(dev())
            pre, mu, rs, delta = ops.edge_pair_fwd(Pa, Pb, cv, W0, meta)
            dPa, dPb, dcv = ops.edge_pair_bwd(dpre, delta, cv, W0, meta, coord=False)
            dPa2, dPb2, dcv2 = ops.edge_pair_bwd(dpre, delta, cv, W0, meta, coord=True)
            got = dict(pre=pre, mu=mu, rs=rs, delta=delta, dPa=dPa, dPb=dPb, dcv=dcv, dcv_coord=dcv2)
            assert torch.equal(dPa, dPa2) and torch.equal(dPb, dPb2)
            for k, t in got.items():
                assert bool(torch.isfinite(t).all()), (k, counts, plant)
            if plant:
                same = (c64(cv)[I] == c64(cv)[J]).all(1)
                assert int(same.sum()) >= sum(c >= 2 for c in counts)
                assert not delta.cpu()[same].any()                       # exactly 0.0
            r64 = _pair_math(Pa, Pb, cv, W0, I, J, dpre, torch.float64)
            r32 = _pair_math(Pa, Pb, cv, W0, I, J, dpre, torch.float32)
            for k, t in got.items():
                held(f"pair H={Hh} vd={vd} counts={counts if len(counts) < 5 else '9x2+3'} plant={plant} {k}",
                     scaled(t, r64[k]), scaled(r32[k], r64[k]), TOL_ELT)


# ---------------------------------------------------------------------------
# B. large logits in attention
# ---------------------------------------------------------------------------
ATTN_FLOORS = (2e-5, 1e-4, 1e-5)        # ctx, dqkv (scaled), lse (absolute): tests/test_attn_tiled_gpu.py


def _attn_run(ops, qkv, dctx, counts, E, heads):
    meta = ops.EdgeMeta.get(counts, dev())
    ctx, lse = ops.attn_fwd(qkv, meta, E, heads)
    return ctx, lse, ops.attn_bwd(qkv, dctx, ctx, lse, meta, E, heads)


def _attn_ref(qkv, dctx, counts, E, heads, dtype):
    q = qkv.detach().cpu().to(dtype).requires_grad_()
    ctx, lse = H.mha64(q, counts, E, heads)
    (ctx * dctx.detach().cpu().to(dtype)).sum().backward()
    return ctx.detach(), lse.detach(), q.grad


def _attn_errs(got, ref):
    return (scaled(got[0], ref[0]), scaled(got[2], ref[2]), float((c64(got[1]) - c64(ref[1])).abs().max()))


def _attn_inputs(counts, E, seed):
    g = torch.Generator().manual_seed(seed)
    R = sum(counts)
    return torch.randn(R, 3 * E, generator=g), torch.randn(R, E, generator=g)


ATTN_CASES = [  # E, heads, option, counts, kernel family that must serve it
    (128, 4, 1, [2, 33, 64], 0), (128, 4, 1, [130, 257], 0),
    (512, 8, 1, [2, 33, 64], 1),
    (512, 8, 2, [2, 33, 64], 2), (512, 8, 2, [130, 257], 2), (512, 8, 1, [130, 257], 2),
]


@pytest.mark.parametrize("E,heads,option,counts,family", ATTN_CASES)
def test_attention_large_logits(ops, E, heads, option, counts, family):
    """q scaled by 8 and by 40: the scores have that spread, and at 40 the row maxima are beyond exp's fp32 overflow.
    ctx, dqkv and lse against torch's MultiheadAttention math in fp64."""
    qkv, dctx = _attn_inputs(counts, E, 1)
    with H.lib_option("attn_tiled", option, default=1):
        assert ops.attn_kernel(E, heads, max(counts)) == family
        for s in (8.0, 40.0):
            x = qkv.clone()
            x[:, :E] *= s
            got = _attn_run(ops, x.to(dev()), dctx.to(dev()), counts, E, heads)
            for t in got:
                assert bool(torch.isfinite(t).all())
            r64, r32 = _attn_ref(x, dctx, counts, E, heads, torch.float64), _attn_ref(x, dctx, counts, E, heads, torch.float32)
            for name, e, y, floor in zip(("ctx", "dqkv", "lse"), _attn_errs(got, r64), _attn_errs(r32, r64), ATTN_FLOORS):
                held(f"attention E={E} family={family} counts={counts} q x {s:g} {name}", e, y, floor)


@pytest.mark.parametrize("E,heads,option,counts,family", ATTN_CASES)
def test_attention_common_key_shift(ops, E, heads, option, counts, family):
    """A constant vector (norm 30 in every head) added to every key row moves all scores of a query together: ctx and dq
    equal the unshifted run's, lse moves by q.c / sqrt(head_dim); and the shifted run holds against fp64 like any other."""
    hd = E // heads
    qkv, dctx = _attn_inputs(counts, E, 2)
    c = torch.randn(heads, hd, generator=torch.Generator().manual_seed(3))
    c = (30.0 * c / c.norm(dim=1, keepdim=True)).reshape(E)
    with H.lib_option("attn_tiled", option, default=1):
        assert ops.attn_kernel(E, heads, max(counts)) == family
        for s in (1.0, 8.0):
            x = qkv.clone()
            x[:, :E] *= s
            y = x.clone()
            y[:, E:2 * E] += c
            base = _attn_run(ops, x.to(dev()), dctx.to(dev()), counts, E, heads)
            got = _attn_run(ops, y.to(dev()), dctx.to(dev()), counts, E, heads)
            r64, r32 = _attn_ref(y, dctx, counts, E, heads, torch.float64), _attn_ref(y, dctx, counts, E, heads, torch.float32)
            yard = _attn_errs(r32, r64)
            tag = f"attention shift E={E} family={family} counts={counts} q x {s:g}"
            for name, e, yd, floor in zip(("ctx", "dqkv", "lse"), _attn_errs(got, r64), yard, ATTN_FLOORS):
                held(f"{tag} {name} vs fp64", e, yd, floor)
            # against the unshifted run of the same kernels (two runs' errors: twice the yardstick)
            held(f"{tag} ctx vs unshifted", scaled(got[0], base[0]), 2 * yard[0], ATTN_FLOORS[0])
            dq_scale = float(c64(base[2]).abs().max())
            e_dq = float((c64(got[2][:, :E]) - c64(base[2][:, :E])).abs().max()) / dq_scale
            held(f"{tag} dq vs unshifted", e_dq, 2 * yard[1], ATTN_FLOORS[1])
            move = (y[:, :E].double().reshape(-1, heads, hd) * c.double().reshape(heads, hd)).sum(-1) / hd ** 0.5
            e_lse = float(((c64(got[1]) - c64(base[1])) - move).abs().max())
            held(f"{tag} lse move", e_lse, 2 * yard[2], ATTN_FLOORS[2])


# ---------------------------------------------------------------------------
# C. LayerNorm rows far from zero
# ---------------------------------------------------------------------------
OFFSETS = (0.0, 1e2, 1e3)
LN_SHAPES = [(3, 16), (37, 32), (9, 264), (5, 4088)]


def _offset_rows(R, D, seed, top):
    """z = m + randn, m constant per row: 0, top / 10, top, with alternating sign, cycling over the rows."""
    g = torch.Generator().manual_seed(seed + R + D)
    m = torch.tensor([(0.0, top / 10, top)[r % 3] * (1 if r % 2 == 0 else -1) for r in range(R)])
    return m[:, None] + torch.randn(R, D, generator=g)


def _affine(D, seed):
    g = torch.Generator().manual_seed(seed + D)
    return 1 + 0.2 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)


def _stats(z, dtype):
    z = z.detach().cpu().to(dtype)
    return z.mean(1), 1.0 / torch.sqrt(z.var(1, unbiased=False) + EPS)


def _act(y, act):
    return y if act == 0 else (torch.relu(y) if act == 1 else torch.nn.functional.gelu(y))


def _ln_formula(z, gamma, beta, act):
    """act((z - mu) * rs * gamma + beta) with mu and rs formed in z's dtype, as the kernels form and store them (not
    torch's fused layer_norm, whose fp32 CPU kernel carries its statistics more precisely than fp32)."""
    mu = z.mean(1, keepdim=True)
    rs = 1.0 / torch.sqrt(((z - mu) ** 2).mean(1, keepdim=True) + EPS)
    return _act((z - mu) * rs * gamma + beta, act)


def _ln(z, gamma, beta, act, dtype):
    return _ln_formula(*(t.detach().cpu().to(dtype) for t in (z, gamma, beta)), act)


def _check_stats(tag, mu, rs, z, floor=TOL_ELT):
    """mu against the row's own magnitude down to its spread (1), rs against itself: fp64 statistics of the fp32 z."""
    (m64, r64), (m32, r32) = _stats(z, torch.float64), _stats(z, torch.float32)
    held(f"{tag} mu", elementwise(mu, m64, 1.0), elementwise(m32, m64, 1.0), floor)
    held(f"{tag} rs", elementwise(rs, r64, 1e-30), elementwise(r32, r64, 1e-30), floor)


@pytest.mark.parametrize("top", OFFSETS[1:])
@pytest.mark.parametrize("R,D", LN_SHAPES)
def test_row_stats_and_layernorm_forward_on_offset_rows(ops, R, D, top):
    z = _offset_rows(R, D, 1, top)
    gamma, beta = _affine(D, 2)
    zd, gd, bd = z.to(dev()), gamma.to(dev()), beta.to(dev())
    mu, rs = ops.row_stats(zd)
    _check_stats(f"row_stats ({R},{D}) m<={top:g}", mu, rs, z)
    for act in (0, 2):
        w64, w32 = _ln(z, gamma, beta, act, torch.float64), _ln(z, gamma, beta, act, torch.float32)
        yard = scaled(w32, w64)
        held(f"ln_act_apply ({R},{D}) m<={top:g} act={act}", scaled(ops.ln_act_apply(zd, mu, rs, gd, bd, act), w64), yard, TOL_ELT)
        if D % 8 == 0:
            mu2, rs2, hs = ops.ln_prep(zd, gd, bd, act)
            _check_stats(f"ln_prep ({R},{D}) m<={top:g}", mu2, rs2, z)
            hi, lo = H.unpack_sx8(hs)
            held(f"ln_prep ({R},{D}) m<={top:g} act={act}", scaled(hi + lo, w64), yard, TOL_ELT)


@pytest.mark.parametrize("top", OFFSETS[1:])
@pytest.mark.parametrize("R,D", LN_SHAPES)
def test_layernorm_backward_on_offset_rows(ops, R, D, top):
    z = _offset_rows(R, D, 3, top)
    gamma, beta = _affine(D, 4)
    dh = torch.randn(R, D, generator=torch.Generator().manual_seed(5))
    zd, gd, bd = z.to(dev()), gamma.to(dev()), beta.to(dev())
    mu, rs = ops.row_stats(zd)
    for act in (0, 2):
        refs = []
        for dtype in (torch.float64, torch.float32):
            zz, g_, b_ = (t.clone().to(dtype).requires_grad_() for t in (z, gamma, beta))
            _ln_formula(zz, g_, b_, act).backward(dh.to(dtype))
            refs.append((zz.grad, g_.grad, b_.grad))
        dz, dg, db, _ = ops.ln_act_bwd(dh.to(dev()), zd, mu, rs, gd, bd, act)
        for name, t, a, b in zip(("dz", "dgamma", "dbeta"), (dz, dg, db), refs[0], refs[1]):
            assert bool(torch.isfinite(t).all())
            held(f"ln_act_bwd ({R},{D}) m<={top:g} act={act} {name}", scaled(t, a), scaled(b, a), 5 * TOL_ELT)


@pytest.mark.parametrize("m", OFFSETS)
@pytest.mark.parametrize("R,K,D", [(5, 8, 8), (37, 3, 64), (7, 5, 264)])
def test_first_layer_with_an_offset_bias(ops, R, K, D, m):
    """z = x W^T + b with b = m + noise: every row of z has mean ~ m."""
    g = torch.Generator().manual_seed(R + K + D)
    x = torch.randn(R, K, generator=g)
    W, b = 0.3 * torch.randn(D, K, generator=g), m + 0.1 * torch.randn(D, generator=g)
    gamma, beta = _affine(D, 6)
    z, mu, rs, hs = ops.first_layer_fwd(x.to(dev()), W.to(dev()), b.to(dev()), gamma.to(dev()), beta.to(dev()), ops.ACT_RELU)
    z64 = x.double() @ W.double().T + b.double()
    held(f"first_layer ({R},{K},{D}) m={m:g} z", scaled(z, z64), scaled(x @ W.T + b, z64), TOL_ELT)
    _check_stats(f"first_layer ({R},{K},{D}) m={m:g}", mu, rs, z)
    hi, lo = H.unpack_sx8(hs)
    w64 = _ln(z, gamma, beta, 1, torch.float64)
    held(f"first_layer ({R},{K},{D}) m={m:g} h", scaled(hi + lo, w64), scaled(_ln(z, gamma, beta, 1, torch.float32), w64), TOL_ELT)


@pytest.mark.parametrize("top", OFFSETS[1:])
@pytest.mark.parametrize("Hh", [64, 260])
def test_pair_statistics_with_offset_rows(ops, Hh, top):
    counts = [5, 2, 7]
    meta = ops.EdgeMeta(counts, dev())
    g = torch.Generator().manual_seed(Hh)
    Pa = _offset_rows(meta.Rv, Hh, 7, top).to(dev())
    Pb = torch.randn(meta.Rv, Hh, generator=g).to(dev())
    cv = torch.randn(meta.Rv, 3, generator=g).to(dev())
    W0 = (0.2 * torch.randn(Hh, 2 * Hh + 7, generator=g)).to(dev())
    pre, mu, rs, _ = ops.edge_pair_fwd(Pa, Pb, cv, W0, meta)
    _check_stats(f"edge_pair_fwd H={Hh} m<={top:g}", mu, rs, pre)


@pytest.mark.parametrize("m", OFFSETS)
@pytest.mark.parametrize("M", [1, 17])
def test_skinny_merged_statistics_with_an_offset_bias(M, m):
    """Y1 = X W1^T + b1 with b1 = m + noise and its per-16-column partials; the next launch merges them (Chan) into
    (mu, rs) and computes Y2 = (relu(LN(Y1)) + A) W2^T + b2 + R.  Bounds of tests/test_skinny_gpu.py as floors."""
    from wf3d import skinny as sk
    K, N1, N2 = 64, 160, 104
    g = torch.Generator().manual_seed(M)
    rn = lambda *s, scale=1.0: torch.randn(*s, generator=g) * scale      # noqa: E731
    X, W1, b1 = rn(M, K), rn(N1, K, scale=K ** -0.5), m + rn(N1)
    ga, be = 1 + 0.1 * rn(N1), 0.1 * rn(N1)
    A, W2, b2, R = rn(M, N1), rn(N2, N1, scale=N1 ** -0.5), rn(N2), rn(M, N2)
    d = lambda t: t.to(dev())      # noqa: E731
    assert sk.ok(M, d(W1), d(W2))
    (Y1, part, _), = sk.fwd(M, sk.Fwd(d(X), d(W1), d(b1), stats=True))
    (Y2, _, (mu, rs)), = sk.fwd(M, sk.Fwd(Y1, d(W2), d(b2), ln=sk.LNIn(d(ga), d(be), 1, part=part), in_add=d(A), out_add=d(R)))
    y64 = X.double() @ W1.double().T + b1.double()
    held(f"skinny M={M} m={m:g} Y1", scaled(Y1, y64), scaled(X @ W1.T + b1, y64), 1e-5)
    _check_stats(f"skinny M={M} m={m:g}", mu, rs, Y1, floor=1e-5)
    y1 = Y1.cpu()

    def second(dtype):
        return (_ln(y1, ga, be, 1, dtype) + A.to(dtype)) @ W2.to(dtype).T + b2.to(dtype) + R.to(dtype)
    held(f"skinny M={M} m={m:g} Y2", scaled(Y2, second(torch.float64)), scaled(second(torch.float32), second(torch.float64)), 1e-5)


# ---------------------------------------------------------------------------
# D. saturated probabilities and exact thresholds
# ---------------------------------------------------------------------------
SPECIAL_P = [0.0, 1.0, 1.0 - 2.0 ** -24, 2.0 ** -149, 1e-30, 0.3]
LOGITS = [0.0, 1e-3, -1e-3, 5.0, -5.0, 20.0, -20.0, 100.0, -100.0, 1e4, -1e4]


def _both_labels(labels):
    """Probabilities for a 0/1 label tensor: every SPECIAL_P value meets a label 0 and a label 1."""
    p = torch.full(labels.shape, 0.3)
    flat_l, flat_p = labels.reshape(-1), p.reshape(-1)
    for want in (0.0, 1.0):
        slots = (flat_l == want).nonzero().reshape(-1).tolist()
        assert len(slots) >= len(SPECIAL_P), (want, len(slots))
        for k, i in enumerate(slots):
            flat_p[i] = SPECIAL_P[k % len(SPECIAL_P)]
    return p


@pytest.mark.parametrize("edge_width", [None, 10, 6])
@pytest.mark.parametrize("assignment", ["device", "scipy"])
def test_loss_at_saturated_probabilities_and_smooth_l1_thresholds(assignment, edge_width):
    """BCE at p = 0, 1, 1 - 2^-24, 2^-149, 1e-30 under both labels (log clamped at -100, gradient denominator at 1e-12:
    gradients of 1e12 / N next to ordinary ones) and SmoothL1 at |d| = 1 exactly and d = 0, against oracle/loss_cpu.py
    (torch's own BCE / SmoothL1 on the CPU).  Losses to 5e-6; every gradient element to 2e-5 of itself + 1e-12."""
    from losses.WireframeLoss import WireframeLoss
    from oracle import loss_cpu
    B, V, counts = 3, 5, [5, 2, 0]
    Ef = V * (V - 1) // 2
    g = torch.Generator().manual_seed(4)
    cnt = torch.tensor(counts)
    # targets on a 2^-10 grid, 10 apart: pred = target +- 1.0 is exact, and the assignment has no near-ties
    tv = torch.round((torch.randn(B, V, 3, generator=g) + 10.0 * torch.arange(V)[None, :, None]) * 1024) / 1024
    pv = tv + torch.round(0.4 * torch.randn(B, V, 3, generator=g) * 1024) / 1024
    pv[0, 0] = tv[0, 0] + torch.tensor([1.0, -1.0, 0.0])
    pv[0, 3] = tv[0, 3] + torch.tensor([0.0, 1.0, 1.0])
    pv[1, 1] = tv[1, 1] + torch.tensor([-1.0, 0.0, -1.0])
    pv[1, 2:] += 100.0                                           # three predictions far from both targets
    te = (torch.arange(V)[None, :] < cnt[:, None]).float()
    tl = (torch.rand(B, Ef, generator=g) > 0.5).float()
    pe, pp = _both_labels(te), _both_labels(tl)
    assert float(pe.min()) == 0.0 and float(pe.max()) == 1.0 and bool((pp == 2.0 ** -149).any())
    tg = {"vertices": tv, "vertex_existence": te, "edge_labels": tl, "vertex_counts": cnt}
    w = pp.shape[1] if edge_width is None else edge_width
    pc = {"vertices": pv.clone().requires_grad_(), "existence_probabilities": pe.clone().requires_grad_(),
          "edge_probs": pp[:, :w].clone().requires_grad_()}
    ref, _ = loss_cpu.wireframe_loss(pc, tg, 3.0, 1.5, 1.0)              # (vertex, edge, existence) weights
    ref["total_loss"].backward()
    pd = {"vertices": pv.to(dev()).requires_grad_(), "existence_probabilities": pe.to(dev()).requires_grad_(),
          "edge_probs": pp.to(dev()).requires_grad_() if edge_width is not None else pp[:, :w].to(dev()).requires_grad_()}
    preds = dict(pd)
    if edge_width is not None:
        preds["edge_width"] = torch.tensor(edge_width, device=dev())
    out = WireframeLoss(3.0, 1.5, 1.0, assignment=assignment)(preds, {k: v.to(dev()) for k, v in tg.items()})
    out["total_loss"].backward()
    for k in ("total_loss", "vertex_loss", "existence_loss", "edge_loss"):
        a, b = float(out[k]), float(ref[k])
        print(f"loss {assignment} width={edge_width} {k}: {a!r} vs {b!r}")
        assert abs(a - b) < 5e-6 * max(1.0, abs(b)), (k, a, b)
    assert float(ref["edge_loss"]) > 10 and float(ref["existence_loss"]) > 10          # the -100 clamps are in play
    for k in pc:
        a, b = pd[k].grad.cpu().double(), pc[k].grad.double()
        assert bool(torch.isfinite(a).all()), k
        if k == "edge_probs" and edge_width is not None:
            assert not a[:, w:].any()                                      # nothing past the device width
            a = a[:, :w]
        worst = float(((a - b).abs() - 2e-5 * b.abs()).max())
        print(f"loss {assignment} width={edge_width} d{k}: |g| in [{float(b.abs().min()):.1e}, {float(b.abs().max()):.1e}], "
              f"worst |a-b| - 2e-5|b| = {worst:.2e} (<= 1e-12)")
        assert worst <= 1e-12, (k, worst)
    assert float(pc["edge_probs"].grad.abs().max()) > 1e9 and float(pc["existence_probabilities"].grad.abs().max()) > 1e9


def _logit_fill(*shape):
    n = 1
    for s in shape:
        n *= s
    return torch.tensor([LOGITS[(i * 7 + i // 11) % len(LOGITS)] for i in range(n)]).reshape(*shape)


def _prob_close(p, logit):
    """fp32 sigmoid = 1 / (1 + exp(-x)) is a few ulp of itself until it underflows (1.2e-38)."""
    want = torch.sigmoid(logit.double())
    bad = (c64(p) - want).abs() - 2e-5 * want - 1e-37
    assert float(bad.max()) <= 0, float(bad.max())


@pytest.mark.parametrize("vd", [4, 6])
@pytest.mark.parametrize("V", [1, 255, 256, 257, 700])
def test_vertex_finalize_at_saturating_logits(ops, V, vd):
    B = 3
    g = torch.Generator().manual_seed(V + vd)
    o = torch.randn(B, V, vd, generator=g)
    o[:, :, 3] = _logit_fill(B, V)
    exist, counts = ops.vertex_finalize_fwd(o.to(dev()), V, vd)
    _prob_close(exist, o[:, :, 3])
    assert torch.equal(counts.cpu(), (o[:, :, 3] > 0).sum(1))                 # logit 0.0 -> 0.5, not counted
    p = exist.cpu()
    if V >= 11:
        assert bool((p == 0).any()) and bool((p == 1).any())
    sat = (p.double() * (1 - p.double())) < 1e-6
    dexist = torch.where(sat, torch.tensor(1e12), torch.randn(B, V, generator=g)) * torch.where(torch.rand(B, V, generator=g) > 0.5, 1.0, -1.0)
    for in_dim in (3, 4):
        d_in = torch.randn(B, V, in_dim, generator=g)
        for de, di in ((dexist, d_in), (None, d_in), (dexist, None)):
            want, mag = torch.zeros(B, V, vd, dtype=torch.float64), torch.zeros(B, V, vd, dtype=torch.float64)
            if di is not None:
                want[:, :, :in_dim] = di.double()
                mag[:, :, :in_dim] = di.double().abs()
            if de is not None:
                term = de.double() * p.double() * (1 - p.double())
                want[:, :, 3] += term
                mag[:, :, 3] += term.abs()
            got = ops.vertex_finalize_bwd(exist, None if de is None else de.to(dev()), None if di is None else di.to(dev()), B, V, vd)
            got = c64(got).reshape(B, V, vd)
            assert bool(torch.isfinite(got).all())
            assert float(((got - want).abs() - 2e-5 * mag).max()) <= 0          # of the two terms' magnitudes: they may cancel
            if de is not None and di is None:
                assert not got[:, :, 3][(p == 0) | (p == 1)].any()         # 1e12 * 0 = exactly 0


def test_edge_prob_at_saturating_logits(ops):
    counts = [4, 2, 7]
    meta = ops.EdgeMeta(counts, dev())
    assert (meta.Re, meta.max_e) == (28, 21)
    logit = _logit_fill(meta.Re, 1)
    probs = ops.edge_prob_fwd(logit.to(dev()), meta)
    p = probs.cpu()
    eoff = meta.eoff.cpu().tolist()
    rows = []
    for s in range(3):
        n = eoff[s + 1] - eoff[s]
        _prob_close(p[s, :n], logit[eoff[s]:eoff[s + 1], 0])
        assert not p[s, n:].any()                                            # padding exactly 0.0
        rows.append(p[s, :n])
    live = torch.cat(rows).double()
    assert bool((live == 0).any()) and bool((live == 1).any())
    g = torch.Generator().manual_seed(1)
    dprobs = torch.where(torch.rand(3, meta.max_e, generator=g) > 0.5, 1e12, -1e12)
    dl = c64(ops.edge_prob_bwd(probs, dprobs.to(dev()), meta)).reshape(-1)
    assert bool(torch.isfinite(dl).all())
    want = torch.cat([dprobs[s, :eoff[s + 1] - eoff[s]] for s in range(3)]).double() * live * (1 - live)
    assert not dl[(live == 0) | (live == 1)].any()
    assert float(((dl - want).abs() - 2e-5 * want.abs()).max()) <= 1e-30


@pytest.mark.parametrize("counts,V", [([4, 2, 7], 7), ([5, 1, 0, 7], 9)])
def test_gather_and_scatter_on_a_strided_view(ops, counts, V):
    B = len(counts)
    meta = ops.EdgeMeta(counts, dev())
    o = torch.randn(B, V, 4, generator=torch.Generator().manual_seed(V))
    view = o.to(dev())[:, :, :3]
    assert not view.is_contiguous()
    cv = ops.edge_gather_verts(view, meta)
    assert torch.equal(cv.cpu(), torch.cat([o[s, :c, :3] for s, c in enumerate(counts)]))
    dcv = torch.randn(meta.Rv, 3, generator=torch.Generator().manual_seed(1))
    dv = ops.edge_scatter_dverts(dcv.to(dev()), meta, B, V).cpu()
    off = 0
    for s, c in enumerate(counts):
        assert torch.equal(dv[s, :c], dcv[off:off + c]) and not dv[s, c:].any()
        off += c
