"""The benchmarked workload held to the fp64 oracle at its own size.

Every number bench.py reports is measured on one workload: train mode, dropout p = 0.1 at the edge head's four sites,
counts = V for every sample, default kernel selection, at bench.CONFIGS.  Several kernel choices depend on the shape
(the pools' split count from (B, N, C), the 32-row skinny head kernels at M = B, MFMA attention at 256 keys, the edge
MLP's TN wgrads over a million edge rows), so the small oracle cases elsewhere in the suite never select some of what
the benchmark runs.  This file runs that workload itself — bench.make_inputs' tensors, the model built as bench.py
builds it — and compares it with the fp64 oracle (oracle/reference_cpu.py) run on the GPU a few samples at a time
(oracle/chunked.py; exact, no operation mixes samples):

a. the bench workload in bf16x3 mode at every config: outputs within 1e-4, every gradient element within TOL_X3 (with
   a documented second yardstick for edge_mlp.4.weight at cfg4 and cfg5: U_X3 below);
b. ragged counts, a zero-padded cloud, non-trivial LayerNorm affines and biases, p = 0 (cfg2, cfg5), same bounds (the
   second yardstick at cfg2);
c. the bench workload in bf16 mode (cfg2, cfg5) at the bf16 bounds of tests/test_precision_bf16_gpu.py;
d. the bench workload in fp32 mode (cfg2, cfg5), forward outputs only.

Gradients are compared decision-frozen (tests/test_frozen_grad_gpu.py): the oracle takes the kernels' own ReLU masks
(read off the sx8 operands of the per-point layers, recomputed for the 32-row head layers, which must then hold no
activation within 5e-7 of 0) and pool arg-max rows, and under dropout the masks oracle/dropout.py replays.  Before any of
that, test_oracle_on_device_matches_cpu holds the device oracle and the chunked runner to the CPU oracle.
"""
import gc
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

import bench  # noqa: E402  (defines constants and functions only)
import helpers as H  # noqa: E402
from helpers import oracle  # noqa: E402
from oracle import dropout as D  # noqa: E402
from oracle.chunked import COT_KEYS, model_forward_chunked  # noqa: E402
from test_frozen_grad_gpu import TOL, TOL_X3  # noqa: E402
from test_precision_bf16_gpu import TOL_BF16_FWD, TOL_BF16_GRAD  # noqa: E402

DROP_P = 0.1                    # bench.py's --dropout default

# Two weight gradients have a second yardstick, in the cases where 2e-4 of max(|g64|, rms g64) was measured to be exceeded
# ("The benchmarked configurations against the oracle"; scripts/debug_edge_wgrad_outliers.py).  Each is
# a product dW = dy^T x summed over rows of the whole batch — edge rows for edge_mlp.4, vertex rows for attention.in_proj —
# whose worst elements are the ones whose terms cancel most (sum_r |dy_ri x_rj| up to 8,000 times the element's
# yardstick), and dy carries the bf16x3 rounding of the edge MLP's split GEMMs.  There an element is held to U_X3 times
# the sum of its own terms' magnitudes — one bf16x3 operand rounding (2^-17) of the product it is — where that is larger
# than TOL_X3 of its yardstick.  Every other tensor, and these in every other case, keep TOL_X3.
U_X3 = 2.0 ** -17
TERMS = {("cfg4", False): ("edge_predictor.edge_mlp.4.weight",),
         ("cfg5", False): ("edge_predictor.edge_mlp.4.weight",),
         ("cfg2", True): ("edge_predictor.edge_mlp.4.weight", "edge_predictor.attention.in_proj_weight")}

ORACLE_BYTES = 3 << 30          # fp64 activations of one oracle chunk (rough budget; the chunk is at least one sample)


def dev():
    return torch.device("cuda:0")


def oracle_chunk(N, V):
    """Samples per oracle chunk: ~15 fp64 values per point and encoder width (Linear, LayerNorm and ReLU outputs of
    5,120 columns kept for backward), ~5,400 per edge row, plus the edge row's dropout masks."""
    per_sample = 8 * (N * 5120 * 3 + V * (V - 1) // 2 * 6200)
    return max(1, ORACLE_BYTES // per_sample)


def free():
    gc.collect()
    torch.cuda.empty_cache()


def drop_seed_from(state):
    """The seed EdgePredictor.forward_ragged draws from torch's generator in `state`."""
    with torch.random.fork_rng(devices=[]):
        torch.set_rng_state(state)
        return int(torch.empty((), dtype=torch.int64).random_().item())


def mask_fn(model, counts, seed, p):
    """(s0, s1) -> the edge-head masks of samples [s0, s1) of the forward that drew `seed` (None for p = 0)."""
    if not p:
        return None
    ep = model.edge_predictor
    counts = [int(c) for c in counts]
    return lambda s0, s1: D.edge_head_masks(seed, counts, (p,) * 4, ep.vertex_proj[4].weight.shape[0], ep._heads, s0, s1)


# ---------------------------------------------------------------------------
# the oracle on the device, chunked, against the CPU oracle
# ---------------------------------------------------------------------------
def test_oracle_on_device_matches_cpu():
    """The fp64 oracle on cuda:0 equals the one on the CPU, and the chunked runner (1 and 2 samples per chunk) the
    unchunked run, to 1e-12 relative on every output and all 76 gradients: ragged counts, a zero-padded cloud, dropout
    0.1 at the four sites, the decisions of a real bf16x3 forward (kernel masks on the encoder)."""
    from models.PointCloudToWireframe import PointCloudToWireframe
    B, N, V, counts = 3, 160, 12, [12, 2, 7]
    torch.manual_seed(11)
    model = PointCloudToWireframe(8, V).to(dev())
    model.vertex_predictor.ensure_point_pool_proj(1024, dev())
    model.set_dropout(DROP_P).train()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, N, 8, generator=g)
    x[0, N - N // 4:] = 0.0
    cnt = torch.tensor(counts)
    state = torch.get_rng_state()
    out = model(x.to(dev()), cnt.to(dev()))
    frozen, _ = H.capture_decisions(out, model, kernel_masks=True, device=dev())
    seed = drop_seed_from(state)
    masks = mask_fn(model, counts, seed, DROP_P)
    cot = {k: torch.randn(out[k].shape, generator=g, dtype=torch.float64) for k in COT_KEYS}
    del out

    def run(device, chunk):
        P = oracle.params_from_module(model, dtype=torch.float64, device=device)
        fz = {"relu": {k: m.to(device) for k, m in frozen["relu"].items()},
              "argmax": {k: a.to(device) for k, a in frozen["argmax"].items()}}
        if chunk is None:
            ref = oracle.model_forward(P, x.double().to(device), cnt, V, training=True, frozen=fz, drop=masks(0, B))
            sum((ref[k] * cot[k].to(device)).sum() for k in COT_KEYS).backward()
        else:
            ref = model_forward_chunked(P, x.double().to(device), cnt, V, chunk, cot=cot, frozen=fz, drop=masks)
        grads = {n: t.grad.cpu().numpy() for n, t in P.items() if t.grad is not None}
        return ref, grads

    ref_cpu, g_cpu = run("cpu", None)
    assert len(g_cpu) == 76
    for tag, (ref, grads) in (("device", run(dev(), None)), ("chunk 1", run(dev(), 1)), ("chunk 2", run(dev(), 2))):
        assert ref["edge_indices"] == ref_cpu["edge_indices"], tag
        fwd = H.out_errs(ref, ref_cpu)
        worst = max(max(a, b) for a, b in fwd.values())
        assert sorted(grads) == sorted(g_cpu), tag
        gw = max(H.elem_err(grads[n], g_cpu[n]) for n in g_cpu)
        print(f"oracle {tag} vs CPU: outputs {worst:.1e}, gradients {gw:.1e}")
        assert worst <= 1e-12 and gw <= 1e-12, (tag, fwd, gw)


# ---------------------------------------------------------------------------
# the bench configurations
# ---------------------------------------------------------------------------
SPIED_OPS = ("gemm", "gemm_split", "gemm_split_tn", "edge_pair_fwd", "ln_prep", "ln_act_apply", "attn_fwd", "pool4_fwd")


@pytest.fixture
def spy(monkeypatch):
    """Records the wf3d.ops and wf3d.skinny calls the model makes, to assert which routes ran."""
    from wf3d import ops, skinny
    calls = []
    for mod, names in ((ops, SPIED_OPS), (skinny, ("fwd", "bwd"))):
        for n in names:
            orig = getattr(mod, n)

            def w(*a, _n=f"{mod.__name__.split('.')[-1]}.{n}", _o=orig, **k):
                calls.append((_n, a, k))
                return _o(*a, **k)
            monkeypatch.setattr(mod, n, w)
    return calls


def routes(calls):
    r = {"skinny_fwd_M": set(), "skinny_bwd_M": set(), "split_rows": [], "tn_rows": [], "pool_rows": [],
         "vp_drop": [], "attn_drop": [], "pair_ln_drop": [], "prep_drop": [], "gemm_drop": []}
    for n, a, k in calls:
        if n == "skinny.fwd":
            r["skinny_fwd_M"].add(a[0])
        elif n == "skinny.bwd":
            r["skinny_bwd_M"].add(a[0])
        elif n == "ops.gemm_split":
            r["split_rows"].append(a[0].shape[0])
        elif n == "ops.gemm_split_tn":
            r["tn_rows"].append(a[0].shape[0])                 # the reduction: rows of the wgrad's operands
        elif n == "ops.pool4_fwd":
            r["pool_rows"].append(tuple(a[0].shape))
        elif n == "ops.ln_act_apply" and k.get("drop_p", 0.0) > 0:
            r["vp_drop"].append(k["drop_p"])
        elif n == "ops.attn_fwd" and a[4] > 0:
            r["attn_drop"].append(a[4])
        elif n == "ops.edge_pair_fwd" and k.get("ln") is not None:
            r["pair_ln_drop"].append(k["ln"][3])
        elif n == "ops.ln_prep" and k.get("drop_p", 0.0) > 0:
            r["prep_drop"].append(k["drop_p"])
        elif n == "ops.gemm" and k.get("pro") is not None and k["pro"].drop_p > 0:
            r["gemm_drop"].append(round(k["pro"].drop_p, 6))
    return r


def check_routes(calls, B, N, V, p, counts, precision):
    """The production route of every choice the Python layer makes at this shape (wf3d/functional.py)."""
    from wf3d import config
    r = routes(calls)
    Re = sum(c * (c - 1) // 2 for c in counts)
    assert r["skinny_fwd_M"] == {B} and r["skinny_bwd_M"] == ({B} if precision != "fp32-fwd" else set()), r
    assert r["pool_rows"] == [(B, N, 512)], r["pool_rows"]
    if precision == "fp32-fwd":
        assert r["split_rows"] == [] and r["tn_rows"] == []
    else:
        # the four per-point Linears after the fused first layer: split GEMMs forward and dgrad, wgrads on the TN kernel
        assert r["split_rows"].count(B * N) == 8, r["split_rows"]
        assert r["tn_rows"].count(B * N) == 4, r["tn_rows"]
    edge_split = precision != "fp32-fwd" and Re >= config.SPLIT_MIN_ROWS
    want = [p] if p else []
    assert r["vp_drop"] == want and [round(v, 6) for v in r["attn_drop"]] == want, r
    if edge_split:
        # the two wide edge-MLP layers: split GEMMs, dropout in the pair kernel's LayerNorm and in ln_prep; their wgrads on
        # the TN kernel wherever it takes the edge-row count (always at counts = V; a ragged count such as 25,672 rows
        # goes through materialised transposes)
        from wf3d import ops
        tn = ops.gemm_split_tn_shape_ok(Re, 256, 512, 256, 512) or ops.gemm_split_tn_shape_ok(Re, 512, 256, 512, 256)
        assert tn or len(set(counts)) > 1, Re
        assert r["split_rows"].count(Re) >= 2 and r["tn_rows"].count(Re) == (2 if tn else 0), (r["split_rows"], r["tn_rows"], Re)
        assert [round(v, 6) for v in r["pair_ln_drop"]] == [p] and [round(v, 6) for v in r["prep_drop"]] == want, r
    else:
        assert r["pair_ln_drop"] == [] and r["tn_rows"].count(Re) == 0
        assert sorted(set(r["gemm_drop"])) == want, r["gemm_drop"]


def bench_model(V, p, perturb=False):
    """The model as bench.py builds it (the caller has set the precision)."""
    from models.PointCloudToWireframe import PointCloudToWireframe
    torch.manual_seed(bench.SEED)
    model = PointCloudToWireframe(input_dim=8, max_vertices=V).to(dev())
    model.vertex_predictor.ensure_point_pool_proj(1024, dev())
    if perturb:
        # LayerNorm affines and biases away from their default init (gamma = 1, beta = 0), as tests/test_frozen_grad_gpu
        with torch.no_grad():
            for n, t in model.named_parameters():
                if t.dim() == 1:
                    t.add_(0.05 * torch.randn(t.shape, generator=torch.Generator().manual_seed(len(n))).to(dev()))
    model.set_dropout(p)
    model.train()
    return model


def bench_inputs(B, N, V, shard, ragged):
    """bench.make_inputs' tensors (shard 0 is what the benchmark times); ragged: counts[0] = V, the others random in
    [2, V], and cloud 0's last quarter zero-padded."""
    x, counts, cot = bench.make_inputs(B, N, V, shard, dev())
    if ragged:
        g = torch.Generator().manual_seed(bench.SEED + shard)
        counts = torch.randint(2, V + 1, (B,), generator=g)
        counts[0] = V
        counts = counts.to(dev())
        x[0, N - N // 4:] = 0.0
    return x, counts, {k: c * (1.0 / B) for k, c in cot.items()}


def report(tag, seed, fwd, errs):
    worst = sorted(((e, n) for n, e in errs.items()), reverse=True)
    print(f"{tag} (input shard {seed}): per-tensor worst element-wise errors")
    for e, n in worst:
        print(f"    {e:.2e}  {n}")
    print("forward (max-abs rel, element-wise):", {k: (f"{a:.1e}", f"{b:.1e}") for k, (a, b) in fwd.items()})


def check_padding(out, counts):
    probs = out["edge_probs"].detach()
    for s, c in enumerate(counts.tolist()):
        e = c * (c - 1) // 2
        if e < probs.shape[1]:
            assert float(probs[s, e:].abs().max()) == 0.0, s


def run_config(spy, cfg, precision, ragged=False, grads=True, shards=4):
    """Runs one case and returns (forward errors, {tensor: elem_err}, {tensor: conditioned error}).  The last holds, for
    the tensors TERMS names for this case, max_ij |g - g64| / max(TOL_X3 max(|g64|, rms g64), U_X3 sum_r |dy_ri x_rj|):
    at most 1 passes.
    A draw whose 32-row head layers hold an activation within 5e-7 of 0 moves to the next input shard (bench.make_inputs
    with the next rank: what a second GPU of the benchmark would time), not to another model seed, so the model stays
    the one bench.py builds."""
    from wf3d import config
    from oracle import reference_cpu
    names = TERMS.get((cfg, ragged), ()) if grads and precision == "bf16x3" else ()
    seen = {}
    B, N, V = bench.CONFIGS[cfg]
    p = 0.0 if ragged else DROP_P
    old = config.precision()
    config.set_precision(precision)
    t0 = time.perf_counter()
    try:
        model = bench_model(V, p, perturb=ragged)
        for shard in range(shards):
            x, counts, cot = bench_inputs(B, N, V, shard, ragged)
            model.zero_grad(set_to_none=True)
            spy.clear()
            state = torch.get_rng_state()
            with torch.set_grad_enabled(grads):
                out = model(x, counts)
            if not grads:
                frozen = None
                break
            frozen, n_border = H.capture_decisions(out, model, kernel_masks=True, device=dev())
            if n_border == 0:
                break
            print(f"{cfg} {precision}: input shard {shard} holds {n_border} head activations within 5e-7 of 0; "
                  f"next shard")
            del out, frozen
        else:
            pytest.fail(f"no borderline-free input in {shards} shards")
        seed = drop_seed_from(state) if p else None
        if grads:
            torch.autograd.backward([out[k] for k in COT_KEYS], [cot[k] for k in COT_KEYS])
        torch.cuda.synchronize()
        check_routes(spy, B, N, V, p, counts.tolist(), precision if grads else "fp32-fwd")
        check_padding(out, counts)
        got = {n: t.grad.detach().cpu().numpy() for n, t in model.named_parameters() if t.grad is not None}
        outs = {k: out[k].detach() for k in ("vertices", "existence_probabilities", "edge_probs", "global_features")}
        indices = out["edge_indices"]
        del out
        free()
        P = oracle.params_from_module(model, dtype=torch.float64, device=dev())
        linear = reference_cpu.F.linear
        if names:
            watched = {id(P[n]): n for n in names}

            def rec(x_, w, b=None):
                y = linear(x_, w, b)
                if id(w) in watched:
                    y.retain_grad()
                    seen.setdefault(watched[id(w)], []).append((x_.detach(), y))
                return y
            reference_cpu.F.linear = rec
        try:
            ref = model_forward_chunked(P, x.double(), counts.cpu(), V, oracle_chunk(N, V),
                                        cot={k: c.double() for k, c in cot.items()} if grads else None,
                                        frozen=frozen, drop=mask_fn(model, counts.tolist(), seed, p))
        finally:
            reference_cpu.F.linear = linear
        assert indices == ref["edge_indices"]
        fwd = H.out_errs(outs, ref)
        errs = {}
        for n, t in P.items():
            if t.grad is None:
                assert n not in got, n
                continue
            errs[n] = H.elem_err(got[n], t.grad.cpu().numpy())
        cond = {}
        for n in names:                                                          # sum_r |dy_ri| |x_rj|
            terms = sum(y.grad.abs().reshape(-1, y.shape[-1]).T @ x_.abs().reshape(-1, x_.shape[-1]) for x_, y in seen[n])
            g64 = P[n].grad
            g = torch.from_numpy(got[n]).to(g64)
            yard = torch.maximum(g64.abs(), g64.square().mean().sqrt())
            cond[n] = float(((g - g64).abs() / torch.maximum(TOL_X3 * yard, U_X3 * terms)).max())
        seen.clear()
        report(f"{cfg} {precision}{' ragged p=0' if ragged else f' p={p}'}", shard, fwd, errs)
        for n, c in cond.items():
            print(f"    {n}: {c:.2f} of max(TOL_X3 of its yardstick, 2^-17 of its terms' magnitudes)")
        print(f"{cfg} {precision}: {time.perf_counter() - t0:.1f} s")
        return fwd, errs, cond
    finally:
        seen.clear()
        config.set_precision(old)
        free()


def check_x3(fwd, errs, cond):
    for k, (a, b) in fwd.items():
        assert a < TOL and b < TOL, (k, a, b)
    assert len(errs) == 76
    bad = [(n, e) for n, e in errs.items() if not (e <= TOL_X3 or cond.get(n, float("inf")) <= 1.0)]
    assert not bad, (bad, cond)


@pytest.mark.parametrize("cfg", ["cfg1", "cfg2", "cfg4", "cfg5"])
def test_bench_workload_bf16x3(spy, cfg):
    """a. exactly what bench.py times at this config."""
    fwd, errs, cond = run_config(spy, cfg, "bf16x3")
    check_x3(fwd, errs, cond)


@pytest.mark.parametrize("cfg", ["cfg2", "cfg5"])
def test_bench_shapes_ragged_bf16x3(spy, cfg):
    """b. the bench shapes with ragged counts (counts[0] = V, the rest random in [2, V]), a zero-padded cloud (the masked
    and unmasked pools differ) and non-trivial LayerNorm affines and biases, no dropout."""
    fwd, errs, cond = run_config(spy, cfg, "bf16x3", ragged=True)
    check_x3(fwd, errs, cond)


@pytest.mark.parametrize("cfg", ["cfg2", "cfg5"])
def test_bench_workload_bf16(spy, cfg):
    """c. the bench workload under set_precision("bf16"), at that mode's bounds."""
    fwd, errs, _ = run_config(spy, cfg, "bf16")
    for k, (a, b) in fwd.items():
        assert a < TOL_BF16_FWD and b < TOL_BF16_FWD, (k, a, b)
    assert len(errs) == 76
    bad = [(n, e) for n, e in errs.items() if not e <= TOL_BF16_GRAD]
    assert not bad, bad


@pytest.mark.parametrize("cfg", ["cfg2", "cfg5"])
def test_bench_workload_fp32_forward(spy, cfg):
    """d. the bench workload in fp32 mode, forward outputs only.  fp32 mode keeps no sx8 operands, so there are no kernel
    masks to freeze the per-point ReLU decisions with, and a full-size batch always holds activations within 5e-7 of 0
    where a recomputed mask could differ from the kernels' own: a decision-frozen gradient check is not meaningful here.
    The forward outputs are continuous in those decisions and are compared with the plain oracle."""
    fwd, errs, _ = run_config(spy, cfg, "fp32", grads=False)
    assert not errs
    for k, (a, b) in fwd.items():
        assert a < TOL and b < TOL, (k, a, b)
