"""The opt-in "bf16" arithmetic mode on the GPU: one bf16 MFMA per product on the hi planes of the sx8 operands.

1. wf3d_gemm_bf16 / wf3d_gemm_bf16_tn against an exact oracle: fp64 products of the HI PLANES decoded from the sx8
   operands themselves (view as bf16, first 8 of every 16).  What is left is fp32 accumulation only, so the bound is
   5e-6 of max |C64| — bf16x3's output misses it by ~2^-9, so the test tells the two arithmetics apart.  Every kernel
   the entry points can select is reached: the persistent and plain 256x256 kernels, the XCD-mapped split-K wgrad,
   dma3, the 256x128 TN kernel, the register-staged fallback (K % 32 != 0) and the variants forced with
   wf3d_set_option("split_kernel", v).
2. - 6. the model in "bf16" mode: golden forward, decision-frozen gradients at the production kernel selection, the
   three-step training trajectory, no state leaking between modes, graph capture.

Bounds TOL_BF16_* were set once, at 2x the first measurement on an MI355X (values beside them and in DESIGN.md §2).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import helpers as H  # noqa: E402  (sys.path)

TOL_ORACLE = 5e-6          # fp32 accumulation of exact bf16 products, relative to max |C64|
M_ENC = 131072             # cfg2: 32 clouds x 4096 points
ROWS_EDGE = 1044480        # cfg5: 32 samples x 32,640 vertex pairs
ENC_LAYERS = [(512, 1024), (1024, 2048), (2048, 1024), (1024, 512)]        # (K_in, N_out) of Linear 2..5

# measured on the first MI355X run, bound = 2x the measured worst value
TOL_BF16_FWD = 1.75e-2     # forward outputs (golden cfg1 / ragged; frozen case), max-abs-relative and element-wise: measured 8.6e-3
TOL_BF16_GRAD = 1.76e-1    # frozen-decision gradients, production selection, worst element: measured 8.78e-2 (attention.in_proj_weight)
TOL_BF16_LOSS0 = 5.5e-3    # traj step-0 loss values and gradient norm, relative: measured 2.75e-3


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from wf3d import ops as o
    o._lib.load()
    return o


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator(device=dev()).manual_seed(seed)
    return torch.randn(*shape, generator=g, device=dev()) * scale


def ints(shape, mul, mod, off):
    n = 1
    for s in shape:
        n *= s
    return ((torch.arange(n, device=dev(), dtype=torch.int64) * mul) % mod - off).float().reshape(shape)


def hi(s):
    """fp64 hi plane of an sx8 matrix [R, C] (any row pitch): per 8 columns, the first 8 of 16 bf16 values."""
    R, C = s.shape
    full = s.as_strided((R, s.stride(0)), (s.stride(0), 1)) if s.stride(0) != C else s
    b = full.contiguous().view(torch.bfloat16).view(R, -1, 16)[:, :, :8].reshape(R, -1)
    return b[:, :C].double()


def err_nt(got, a_s, b_s, bias=None, addend=None, chunk=16384):
    """max |got - (hi(A) hi(B)^T + bias + addend)| / max |ref| over every element (fp64, row chunks)."""
    Bd = hi(b_s)
    err = torch.zeros((), dtype=torch.float64, device=dev())
    top = torch.zeros((), dtype=torch.float64, device=dev())
    for r in range(0, a_s.shape[0], chunk):
        want = hi(a_s[r:r + chunk]) @ Bd.T
        if bias is not None:
            want += bias.double()
        if addend is not None:
            want += addend[r:r + chunk].double()
        err = torch.maximum(err, (got[r:r + chunk].double() - want).abs().max())
        top = torch.maximum(top, want.abs().max())
    return float(err / top), float(err)


def err_tn(got, a_s, b_s, chunk=16384):
    """the same for C = A^T B (A = sx8[K, Mo], B = sx8[K, No])."""
    want = torch.zeros(a_s.shape[1], b_s.shape[1], dtype=torch.float64, device=dev())
    for r in range(0, a_s.shape[0], chunk):
        want += hi(a_s[r:r + chunk]).T @ hi(b_s[r:r + chunk])
    err = (got.double() - want).abs().max()
    return float(err / want.abs().max()), float(err)


# ---------------------------------------------------------------------------------------------------------------------
# 1. kernels against the exact hi-plane oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,N", ENC_LAYERS)
def test_bf16_forward_and_dgrad_at_encoder_launch_shapes(ops, K, N):
    """persistent 256x256 kernel (bias as accumulator start, and without bias) and the dgrad dz·W at M = 131,072."""
    M = M_ENC
    W = rnd(N, K, seed=2, scale=0.05)
    As, Ws, bias = ops.split_rows(rnd(M, K, seed=1)), ops.split_rows(W), rnd(N, seed=3)
    got = ops.gemm_split(As, Ws, bias=bias, products=1)
    r, _ = err_nt(got, As, Ws, bias)
    assert r < TOL_ORACLE, f"forward K={K} N={N}: {r:.2e}"
    x3 = ops.gemm_split(As, Ws, bias=bias)                               # the arithmetic differs: bf16x3 misses the bound
    r3, _ = err_nt(x3, As, Ws, bias)
    assert r3 > 20 * TOL_ORACLE, f"bf16x3 output within {r3:.2e} of the hi-plane oracle"
    del x3
    got2 = ops.gemm_split(As, Ws, products=1)
    assert torch.equal(got2, ops.gemm_split(As, Ws, products=1, out=torch.full_like(got2, 7.0)))     # bit-identical rerun
    r, _ = err_nt(got2, As, Ws)
    assert r < TOL_ORACLE
    del got, got2, As
    Gs, WTs = ops.split_rows(rnd(M, N, seed=4)), ops.split_rows(W, transpose=True)
    dh = ops.gemm_split(Gs, WTs, products=1)
    r, _ = err_nt(dh, Gs, WTs)
    assert r < TOL_ORACLE, f"dgrad K={N} N={K}: {r:.2e}"


@pytest.mark.parametrize("Mo,No", [(1024, 512), (2048, 1024), (1024, 2048), (512, 1024)])
def test_bf16_wgrad_at_encoder_launch_shapes(ops, Mo, No):
    """dW = dz^T·h over K = 131,072 rows: XCD-mapped split-K of the 256x256 transposing-read kernel + slab fold."""
    K = M_ENC
    dzs, hs = ops.split_rows(rnd(K, Mo, seed=5)), ops.split_rows(rnd(K, No, seed=6).relu_())
    assert ops.gemm_split_tn_ok(dzs, hs)
    got = ops.gemm_split_tn(dzs, hs, products=1)
    r, _ = err_tn(got, dzs, hs)
    assert r < TOL_ORACLE, f"wgrad {Mo}x{No}: {r:.2e}"
    assert torch.equal(got, ops.gemm_split_tn(dzs, hs, products=1))
    r3, _ = err_tn(ops.gemm_split_tn(dzs, hs), dzs, hs)
    assert r3 > 20 * TOL_ORACLE


@pytest.mark.parametrize("K,N", [(512, 256), (256, 128)])
def test_bf16_edge_mlp_gemms_at_cfg5_row_count(ops, K, N):
    """1,044,480 pair rows through Linear(512,256) / Linear(256,128): forward, dgrad, few-tile wgrad."""
    R = ROWS_EDGE
    As, Ws, bias = ops.split_rows(rnd(R, K, seed=7)), ops.split_rows(rnd(N, K, seed=8, scale=0.05)), rnd(N, seed=9)
    got = ops.gemm_split(As, Ws, bias=bias, products=1)
    r, _ = err_nt(got, As, Ws, bias)
    assert r < TOL_ORACLE, f"edge forward {K}->{N}: {r:.2e}"
    del got
    Gs = ops.split_rows(rnd(R, N, seed=10))
    WTs = ops.split_rows(rnd(N, K, seed=8, scale=0.05), transpose=True)
    dh = ops.gemm_split(Gs, WTs, products=1)
    r, _ = err_nt(dh, Gs, WTs)
    assert r < TOL_ORACLE, f"edge dgrad {N}->{K}: {r:.2e}"
    del dh
    if ops.gemm_split_tn_ok(Gs, As):
        got = ops.gemm_split_tn(Gs, As, products=1)
        r, _ = err_tn(got, Gs, As)
    else:                                                                 # the transposed problem, as functional._wgrad does ("tn_t")
        got = ops.gemm_split_tn(As, Gs, products=1)
        r, _ = err_tn(got, As, Gs)
    assert r < TOL_ORACLE, f"edge wgrad {N}x{K}: {r:.2e}"


@pytest.mark.parametrize("M,N,K", [(1000, 384, 256), (4096, 256, 512), (300, 40, 64)])
def test_bf16_few_tile_kernels(ops, M, N, K):
    """problems with < 192 tiles: dma3 (256x128 tiles, split-K below 192 tiles), partial row / column tiles."""
    As, Ws, bias = ops.split_rows(rnd(M, K, seed=11)), ops.split_rows(rnd(N, K, seed=12, scale=0.1)), rnd(N, seed=13)
    got = ops.gemm_split(As, Ws, bias=bias, products=1)
    r, _ = err_nt(got, As, Ws, bias)
    assert r < TOL_ORACLE, (M, N, K, r)


@pytest.mark.parametrize("K,Mo,No", [(4096, 256, 128), (2048, 512, 384), (64, 256, 128)])
def test_bf16_tn_kernel_256x128(ops, K, Mo, No):
    """outputs that are not multiples of 256 wide: the 256x128 TN kernel (split-K over long K)."""
    As, Bs = ops.split_rows(rnd(K, Mo, seed=14)), ops.split_rows(rnd(K, No, seed=15))
    got = ops.gemm_split_tn(As, Bs, products=1)
    r, _ = err_tn(got, As, Bs)
    assert r < TOL_ORACLE, (K, Mo, No, r)


@pytest.mark.parametrize("M,N,K", [(1000, 200, 40), (257, 128, 72), (64, 64, 8)])
def test_bf16_register_staged_fallback(ops, M, N, K):
    """K not a multiple of 32: the DMA kernels refuse, the register-staged gemm_kernel<..., SPLIT> takes it."""
    assert K % 32 != 0
    As, Ws, bias = ops.split_rows(rnd(M, K, seed=16)), ops.split_rows(rnd(N, K, seed=17, scale=0.1)), rnd(N, seed=18)
    got = ops.gemm_split(As, Ws, bias=bias, products=1)
    r, _ = err_nt(got, As, Ws, bias)
    assert r < TOL_ORACLE, (M, N, K, r)


@pytest.mark.parametrize("M,N,K", [(131072, 1024, 512), (5000, 512, 256), (1000, 200, 40)])
def test_bf16_pitch_bias_accumulate(ops, M, N, K):
    """lda > K (operands are column slices of wider sx8 matrices), an accumulating call on top of a bias call, M not a
    multiple of 256 — through the persistent kernel's refusal (accumulate), the plain and dma3 kernels, the fallback."""
    Af, Wf = ops.split_rows(rnd(M, K + 32, seed=19)), ops.split_rows(rnd(N, K + 64, seed=20, scale=0.05))
    As, Ws, bias = Af[:, :K], Wf[:, :K], rnd(N, seed=21)
    assert As.stride(0) == K + 32 and Ws.stride(0) == K + 64
    C0 = rnd(M, N, seed=22)
    out = C0.clone()
    ops.gemm_split(As, Ws, bias=bias, out=out, accumulate=True, products=1)
    r, _ = err_nt(out, As, Ws, bias, addend=C0)
    assert r < TOL_ORACLE, (M, N, K, r)


@pytest.mark.parametrize("K,N", ENC_LAYERS[:2])
def test_bf16_exact_on_integer_data(ops, K, N):
    """small integers are exact in bf16 (hi = v, lo = 0) and every fp32 partial sum is exact: a slice dropped, doubled
    or mis-addressed shows bit-exactly; forward, dgrad and wgrad at the cfg2 launch shapes."""
    M = M_ENC
    A, W, bias = ints((M, K), 1, 11, 5), ints((N, K), 7, 13, 6), ints((N,), 1, 5, 2)
    As, Ws = ops.split_rows(A), ops.split_rows(W)
    got = ops.gemm_split(As, Ws, bias=bias, products=1)
    _, err = err_nt(got, As, Ws, bias)
    assert err == 0.0
    assert torch.equal(got, ops.gemm_split(As, Ws, bias=bias, products=1))
    dz, h = ints((M, N), 1, 5, 2), ints((M, K), 3, 7, 3)
    got = ops.gemm_split_tn(ops.split_rows(dz), ops.split_rows(h), products=1)
    _, err = err_tn(got, ops.split_rows(dz), ops.split_rows(h))
    assert err == 0.0


@pytest.mark.parametrize("kernel", [3, 6, 1])
def test_bf16_forced_variants(ops, kernel):
    """split_kernel = 3 / 6 / 1: every problem through dma3, the 256x256 kernels, or the register-staged one."""
    worst = 0.0
    with H.lib_option("split_kernel", kernel):
        for (M, N, K) in [(4096, 512, 256), (65536, 1024, 512), (1000, 384, 128)]:
            As, Ws, b = ops.split_rows(rnd(M, K, seed=1)), ops.split_rows(rnd(N, K, seed=2, scale=0.1)), rnd(N, seed=3)
            worst = max(worst, err_nt(ops.gemm_split(As, Ws, bias=b, products=1), As, Ws, b)[0])
    assert worst < TOL_ORACLE, (kernel, worst)


# ---------------------------------------------------------------------------------------------------------------------
# 2. - 6. the model in "bf16" mode
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def bf16_forced():
    """"bf16" mode with every eligible Linear on the split path, also at the golden fixtures' small sizes."""
    from wf3d import config
    old = (config.precision(), config.SPLIT_MIN_ROWS)
    config.set_precision("bf16")
    config.SPLIT_MIN_ROWS = 1
    yield
    config.set_precision(old[0])
    config.SPLIT_MIN_ROWS = old[1]


@pytest.mark.parametrize("tag", ["cfg1", "ragged"])
def test_bf16_model_forward_vs_golden(tag, bf16_forced):
    from test_model_gpu import build_full
    gold, model, x, arrs, counts, V, seed, train = build_full(tag)
    with torch.set_grad_enabled(train):
        out = model(torch.from_numpy(x).to(dev()), counts.to(dev()) if counts is not None else None)
    lens = [len(e) for e in out["edge_indices"]]
    assert lens == gold["out.edge_index_lens"].tolist()
    flat = np.array([ij for e in out["edge_indices"] for ij in e], dtype=np.int64).reshape(-1, 2)
    assert np.array_equal(flat, gold["out.edge_indices_flat"])                   # bit-exact
    worst = {}
    for k in ("vertices", "existence_probabilities", "edge_probs", "global_features"):
        got = out[k].detach().cpu().numpy()
        worst[k] = max(H.rel_err(got, gold["out." + k]), H.elem_err(got, gold["out." + k], H.OUT_FLOOR[k]))
    print(f"MEASURED bf16 forward {tag}:", {k: f"{v:.2e}" for k, v in worst.items()})
    for k, v in worst.items():
        assert v < TOL_BF16_FWD, (k, v)
    ep = out["edge_probs"].detach().cpu().numpy()
    for s, n in enumerate(lens):
        assert np.all(ep[s, n:] == 0.0)


def test_bf16_frozen_gradients_production_kernel_selection():
    """B=8, N=4096, V=64, default SPLIT_MIN_ROWS: the kernels the benchmark runs, every element of every gradient against
    fp64 under the kernels' own decisions.  Prints the per-tensor worst-element table (profiles/r04_precision_grad_table.txt)."""
    from test_frozen_grad_gpu import _run
    counts = [64, 33, 2, 7, 50, 64, 12, 40]
    fwd, errs, seed = _run("bf16", 8, 4096, 64, counts, min_rows=None, kernel_masks=True, draws=8)
    worst = sorted(((e, n) for n, e in errs.items()), reverse=True)
    print(f"bf16, production kernel selection (input seed {seed}): per-tensor worst element-wise errors")
    for e, n in worst:
        print(f"    {e:.2e}  {n}")
    print("MEASURED bf16 frozen forward (max-abs rel, element-wise):", {k: (f"{a:.1e}", f"{b:.1e}") for k, (a, b) in fwd.items()})
    print(f"MEASURED bf16 frozen worst gradient element: {worst[0][0]:.3e} ({worst[0][1]})")
    assert len(errs) == 76
    for k, (a, b) in fwd.items():
        assert a < TOL_BF16_FWD and b < TOL_BF16_FWD, (k, a, b)
    bad = [(n, e) for n, e in errs.items() if not e <= TOL_BF16_GRAD]
    assert not bad, bad


def test_bf16_three_step_trajectory_with_device_loss():
    """tests/golden/traj.npz (three train.py-ordered steps of the reference) in "bf16" mode with the device loss, every
    eligible Linear on the one-product path: step 0 within the measured bound, later steps within the spread the
    reference itself shows (3e-2 / 1.5e-1, as tests/test_train_loop_gpu.py allows)."""
    from oracle import detgen
    from wf3d import config
    from losses.WireframeLoss import WireframeLoss
    from models.PointCloudToWireframe import PointCloudToWireframe
    g = H.load_golden("traj")
    seed, (B, N, V), counts = int(g["meta.seed"]), [int(v) for v in g["meta.dims"]], g["meta.counts"]
    x = detgen.normalish("traj.x", (B, N, 8), seed)
    x[1, ::5] = 0.0
    tv = 0.5 * detgen.normalish("traj.tv", (B, V, 3), seed)
    te = (np.arange(V)[None, :] < counts[:, None]).astype(np.float32)
    tl = (detgen.uniform("traj.tl", (B, V * (V - 1) // 2), 0, 1, seed) > 0.75).astype(np.float32)
    old = (config.precision(), config.SPLIT_MIN_ROWS)
    config.set_precision("bf16")
    config.SPLIT_MIN_ROWS = 1
    try:
        torch.manual_seed(seed)
        model = PointCloudToWireframe(input_dim=8, max_vertices=V).to(dev()).set_dropout(0.0)
        opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-6)
        crit = WireframeLoss(vertex_weight=3.0, edge_weight=1.5, existence_weight=1.0, assignment="device")
        xt, cnt = torch.from_numpy(x).to(dev()), torch.from_numpy(counts).to(dev())
        tgts = {"vertices": torch.from_numpy(tv).to(dev()), "vertex_existence": torch.from_numpy(te).to(dev()),
                "edge_labels": torch.from_numpy(tl).to(dev()), "vertex_counts": cnt}
        model.train()
        step0 = 0.0
        for step, want in enumerate(g["traj"]):
            opt.zero_grad()
            out = model(xt, cnt)
            losses = crit(out, tgts)
            losses["total_loss"].backward()
            gn = torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=1.0)
            opt.step()
            got = [float(losses[k].detach()) for k in ("total_loss", "vertex_loss", "existence_loss", "edge_loss")] + [float(gn)]
            for name, a, b in zip(("total", "vertex", "existence", "edge", "grad_norm"), got, want):
                rel = abs(a - b) / max(1.0, abs(b))
                if step == 0:
                    step0 = max(step0, rel)
                    tol = TOL_BF16_LOSS0
                else:
                    tol = (3e-2, 1.5e-1)[step - 1] * (3 if name == "grad_norm" else 1)
                assert rel <= tol, (step, name, a, b)
        print(f"MEASURED bf16 traj step-0 worst relative loss / grad-norm error: {step0:.3e}")
    finally:
        config.set_precision(old[0])
        config.SPLIT_MIN_ROWS = old[1]


def _loss(o):
    return o["vertices"].sum() + o["existence_probabilities"].sum() + o["edge_probs"].sum()


@pytest.fixture(scope="module")
def small():
    from models.PointCloudToWireframe import PointCloudToWireframe
    torch.manual_seed(0)
    m = PointCloudToWireframe(8, 6).to(dev())
    m.vertex_predictor.ensure_point_pool_proj(1024, dev())
    m.set_dropout(0.0)
    m.train()
    x = torch.randn(3, 300, 8, device=dev())
    c = torch.tensor([6, 2, 4], device=dev())
    return m, x, c


def _fwd_bwd(m, x, c):
    m.zero_grad(set_to_none=True)
    out = m(x, c)
    _loss(out).backward()
    return ({k: out[k].detach().clone() for k in ("vertices", "existence_probabilities", "edge_probs")},
            {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None})


def test_no_leak_between_modes(small):
    """bf16x3, then bf16, then bf16x3 again: the two bf16x3 runs are bit-identical; bf16 differs (it ran).  The forward's
    product count travels with the autograd context: a mode switch between forward and backward does not change the
    backward, and PointNetEncoder.precision = "bf16" overrides the global mode like the other values."""
    from wf3d import config
    m, x, c = small
    old = (config.precision(), config.SPLIT_MIN_ROWS)
    config.SPLIT_MIN_ROWS = 1
    try:
        config.set_precision("bf16x3")
        o1, g1 = _fwd_bwd(m, x, c)
        config.set_precision("bf16")
        ob, gb = _fwd_bwd(m, x, c)
        config.set_precision("bf16x3")
        o2, g2 = _fwd_bwd(m, x, c)
        for k in o1:
            assert torch.equal(o1[k], o2[k]), k
        for n in g1:
            assert torch.equal(g1[n], g2[n]), n
        assert not torch.equal(o1["vertices"], ob["vertices"])
        assert any(not torch.equal(g1[n], gb[n]) for n in g1)
        # mode switched between forward and backward: backward still runs the forward's arithmetic
        config.set_precision("bf16")
        m.zero_grad(set_to_none=True)
        out = m(x, c)
        config.set_precision("bf16x3")
        _loss(out).backward()
        for n, p in m.named_parameters():
            if p.grad is not None:
                assert torch.equal(p.grad, gb[n]), n
        # per-module override
        m.encoder.precision = "bf16"
        try:
            g_over = m.encoder.encode(x)[0].detach().clone()
        finally:
            m.encoder.precision = None
        config.set_precision("bf16")
        assert torch.equal(g_over, m.encoder.encode(x)[0].detach())
    finally:
        config.set_precision(old[0])
        config.SPLIT_MIN_ROWS = old[1]


def test_bf16_step_is_capturable_into_a_graph(small):
    """a whole bf16-mode step captured with torch.cuda.graph replays bit-identical to eager."""
    from wf3d import config
    m, x, c = small
    old = (config.precision(), config.SPLIT_MIN_ROWS)
    config.set_precision("bf16")
    config.SPLIT_MIN_ROWS = 1
    try:
        def step():
            for p in m.parameters():
                p.grad = None
            _loss(m(x, c)).backward()

        s = torch.cuda.Stream(x.device)
        s.wait_stream(torch.cuda.current_stream(x.device))
        with torch.cuda.stream(s):
            for _ in range(2):
                step()
        torch.cuda.current_stream(x.device).wait_stream(s)
        torch.cuda.synchronize()
        eager = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            step()
        grads = {n: p.grad for n, p in m.named_parameters() if p.grad is not None}
        for _ in range(2):
            g.replay()
        torch.cuda.synchronize()
        assert set(grads) == set(eager)
        for n in eager:
            assert torch.equal(grads[n], eager[n]), n
        for p in m.parameters():
            p.grad = None
    finally:
        config.set_precision(old[0])
        config.SPLIT_MIN_ROWS = old[1]
