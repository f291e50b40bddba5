"""Packed point-cloud batches on the GPU: the segmented pool kernels alone, PointCloudToWireframe.forward_packed against
tests/golden/packed.npz (the reference on each cloud alone) and against the decision-frozen fp64 oracle, and what sets a
packed batch apart from a zero-padded one.  The tolerances are the project's own (tests/test_model_gpu.py,
tests/test_frozen_grad_gpu.py, tests/test_precision_bf16_gpu.py, tests/test_kernels_gpu.py)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import helpers as H  # noqa: E402
from helpers import oracle  # noqa: E402
from test_packed import packed_case, packed_cotangents  # noqa: E402

TOL_OUT = 1e-4              # tests/test_model_gpu.py
TOL_GRAD = 1e-3
TOL = 1e-4                  # tests/test_frozen_grad_gpu.py: fp32, every gradient element
TOL_X3 = 2e-4               # bf16x3, production kernel selection
TOL_BF16_FWD = 1.75e-2      # tests/test_precision_bf16_gpu.py
TOL_BF16_GRAD = 1.76e-1
OUT_KEYS = ("vertices", "existence_probabilities", "edge_probs", "global_features")


def dev():
    return torch.device("cuda:0")


@pytest.fixture
def ops():
    from wf3d import ops as o
    return o


def rel(a, b):
    return H.rel_err(a.detach().cpu().numpy(), b.detach().cpu().numpy())


@pytest.fixture
def mode(request):
    """(precision, SPLIT_MIN_ROWS) for the body of a test; the split modes are forced onto small shapes by min_rows = 1."""
    from wf3d import config
    old = (config.precision(), config.SPLIT_MIN_ROWS)
    precision, min_rows = request.param
    config.set_precision(precision)
    if min_rows is not None:
        config.SPLIT_MIN_ROWS = min_rows
    yield precision
    config.set_precision(old[0])
    config.SPLIT_MIN_ROWS = old[1]


FORCED = [("fp32", 1), ("bf16x3", 1), ("bf16", 1)]


# ---------------------------------------------------------------------------------------------------------------------
# the segmented pool kernels alone
# ---------------------------------------------------------------------------------------------------------------------
def _seg_inputs(ops, C, counts, seed=0):
    """pf [M_pad, C] with planted ties, valid [M_pad] (some rows invalid, the one-point cloud dead), the layout.
    The pad rows of pf hold NaN: a forward that read them would show it."""
    lay = ops.PackedLayout.get(counts, dev())
    g = torch.Generator().manual_seed(seed)
    pf = torch.randn(lay.M_pad, C, generator=g)
    valid = (torch.rand(lay.M_pad, generator=g) > 0.2).float()
    for b, n in enumerate(counts):
        o = int(lay.offsets[b])
        if n == 1:
            valid[o] = 0.0                                   # a dead cloud
        if n >= 5:
            # equal maxima: columns 0..C/2 reach 50 in rows 1 and 3 (and 4096 of a long cloud, another chunk)
            rows = [1, 3] + ([4096] if n > 4096 else [])
            for r in rows:
                pf[o + r, :C // 2] = 50.0
            valid[o + 1] = 0.0                               # the first of them is masked out: the masked arg-max is row 3
            valid[o + 3] = 1.0
    pf[lay.M:] = float("nan")
    valid[lay.M:] = 0.0
    return lay, pf.to(dev()), valid.to(dev())


def _first_max(seg, ok):
    """(max over the rows where ok, index of its first occurrence) per column; (0, -1) where no row is ok."""
    n = seg.shape[0]
    neg = torch.full_like(seg, float("-inf"))
    s = torch.where(ok[:, None], seg, neg)
    mx = s.max(dim=0).values
    ar = torch.arange(n, device=seg.device)[:, None].expand_as(seg)
    idx = torch.where((s == mx[None]) & ok[:, None], ar, torch.full_like(ar, n)).min(dim=0).values
    none = ~ok.any()
    return (torch.zeros_like(mx) if none else mx), (torch.full_like(idx, -1) if none else idx)


SEG_CASES = [(512, [1, 5, 300, 4097]), (520, [1, 5, 300, 4097]), (64, [1, 5, 300, 4097]), (512, [256, 256]), (64, [7000, 3])]


@pytest.mark.parametrize("C,counts", SEG_CASES)
def test_seg_pool_forward_vs_per_cloud_restatement(ops, C, counts):
    lay, pf, valid = _seg_inputs(ops, C, counts)
    po = ops.pool4_seg_fwd(pf, valid, lay)
    for b, n in enumerate(counts):
        o = int(lay.offsets[b])
        seg, ok = pf[o:o + n], valid[o:o + n] != 0
        mmax, am = _first_max(seg, ok)
        umax, au = _first_max(seg, torch.ones_like(ok))
        assert torch.equal(po.mmax[b], mmax) and torch.equal(po.arg_m[b].long(), am), b           # exact, ties included
        assert torch.equal(po.umax[b], umax) and torch.equal(po.arg_u[b].long(), au), b
        if n >= 5:
            assert int(po.arg_u[b, 0]) == 1 and int(po.arg_m[b, 0]) == 3                          # the planted ties
        nv = float(ok.sum())
        assert float(po.nvalid[b]) == nv and float(po.cnt[b]) == max(nv, 1.0)
        s64 = seg.double()
        assert rel(po.umean[b], s64.mean(0)) < 1e-6, b                                            # divides by N_b
        mavg = (s64 * ok[:, None]).sum(0) / max(nv, 1.0)
        assert (po.mavg[b].double() - mavg).abs().max() <= 1e-6 * max(float(mavg.abs().max()), 1e-30), b
    assert torch.isfinite(po.masked).all() and torch.isfinite(po.unmasked).all()                  # pad rows were not read
    po2 = ops.pool4_seg_fwd(pf, valid, lay)
    assert torch.equal(po.masked, po2.masked) and torch.equal(po.unmasked, po2.unmasked)          # deterministic


def _seg_backward_reference(pf, valid, lay, po, cots, direct):
    """autograd of the per-cloud restatement in fp64 (arg-max rows: the forward's, verified exact above)."""
    x = pf[:lay.M].double().requires_grad_()
    tot = 0.0
    for b, n in enumerate(lay.counts):
        o = int(lay.offsets[b])
        seg, ok = x[o:o + n], valid[o:o + n].double()
        cols = torch.arange(seg.shape[1], device=pf.device)
        am, au = po.arg_m[b].long(), po.arg_u[b].long()
        mmax = torch.where(am >= 0, seg[am.clamp(min=0), cols], torch.zeros_like(seg[0]))
        umax = seg[au, cols]
        mavg = (seg * ok[:, None]).sum(0) / po.cnt[b].double()
        umean = seg.mean(0)
        tot = tot + sum((c[b].double() * v).sum() for c, v in zip(cots, (mmax, mavg, umean, umax)))
    if direct is not None:
        tot = tot + (x * direct.double()).sum()
    tot.backward()
    return x.grad


@pytest.mark.parametrize("C,counts", SEG_CASES)
def test_seg_pool_backward_three_forms(ops, C, counts):
    lay, pf, valid = _seg_inputs(ops, C, counts)
    po = ops.pool4_seg_fwd(pf, valid, lay)
    g = torch.Generator().manual_seed(5)
    B, M = lay.B, lay.M
    dm = torch.randn(B, 2 * C, generator=g).to(dev())         # strided halves of [B, 2C] gradients, as the encoder passes them
    du = torch.randn(B, 2 * C, generator=g).to(dev())
    cots = (dm[:, :C], dm[:, C:], du[:, :C], du[:, C:])
    direct = torch.randn(M, C, generator=g).to(dev())
    pf0 = torch.nan_to_num(pf, nan=0.0)
    for d in (None, direct):
        dpf = ops.pool4_seg_bwd(valid, po.cnt, po.arg_m, po.arg_u, *cots, d, lay, C)
        assert dpf.shape == (lay.M_pad, C)
        want = _seg_backward_reference(pf0, valid, lay, po, cots, d)
        assert rel(dpf[:M], want) < 1e-6
        assert lay.M_pad == M or float(dpf[M:].abs().max()) == 0.0                # pad rows: exact zeros
        cs = ops.pool4_seg_bwd_colsum(po.nvalid, po.cnt, po.arg_m, po.arg_u, *cots, d, lay, C)
        assert rel(cs, dpf.double().sum(0)) < 1e-5                                  # the bias column sum
        if C % 8 == 0:
            s8 = ops.pool4_seg_bwd(valid, po.cnt, po.arg_m, po.arg_u, *cots, d, lay, C, sx8=True)
            hi, lo = H.unpack_sx8(s8)
            assert torch.equal(hi, dpf.bfloat16().float())                          # the RNE split of the fp32 form,
            assert torch.equal(lo, (dpf - hi).bfloat16().float())                   # both planes
            assert rel(hi + lo, dpf) < 2e-5                                         # the split format's 2^-17
            assert lay.M_pad == M or (float(hi[M:].abs().max()) == 0.0 and float(lo[M:].abs().max()) == 0.0)
    # no cotangent for one of the pairs
    none = (None, None, cots[2], cots[3])
    dpf = ops.pool4_seg_bwd(valid, po.cnt, po.arg_m, po.arg_u, *none, None, lay, C)
    zero = torch.zeros(B, C, device=dev())
    assert rel(dpf[:M], _seg_backward_reference(pf0, valid, lay, po, (zero, zero, cots[2], cots[3]), None)) < 1e-6


def test_seg_pool_equals_dense_pool_at_equal_lengths(ops):
    B, N, C = 8, 512, 512
    lay = ops.PackedLayout.get([N] * B, dev())
    g = torch.Generator().manual_seed(2)
    pf = torch.randn(B * N, C, generator=g).to(dev())
    valid = (torch.rand(B * N, generator=g) > 0.3).float().to(dev())
    a, d = ops.pool4_seg_fwd(pf, valid, lay), ops.pool4_fwd(pf.view(B, N, C), valid, packed=True)
    assert torch.equal(a.mmax, d.mmax) and torch.equal(a.umax, d.umax)
    assert torch.equal(a.arg_m, d.arg_m) and torch.equal(a.arg_u, d.arg_u) and torch.equal(a.cnt, d.cnt)
    assert rel(a.mavg, d.mavg) < 1e-6 and rel(a.umean, d.umean) < 1e-6
    cot = torch.randn(B, 2 * C, generator=g).to(dev())
    args = (valid, d.cnt, d.arg_m, d.arg_u, cot[:, :C], cot[:, C:], cot[:, C:], cot[:, :C], None)
    assert torch.equal(ops.pool4_seg_bwd(*args, lay, C), ops.pool4_bwd(*args, B, N, C).view(B * N, C))
    assert torch.equal(ops.pool4_seg_bwd(*args, lay, C, sx8=True), ops.pool4_bwd(*args, B, N, C, sx8=True).view(B * N, C))


# ---------------------------------------------------------------------------------------------------------------------
# the whole model
# ---------------------------------------------------------------------------------------------------------------------
def build_packed():
    from models.PointCloudToWireframe import PointCloudToWireframe
    from test_model_gpu import load_arrays
    from wf3d.packed import pack
    gold, clouds, arrs, counts, V, seed = packed_case()
    model = PointCloudToWireframe(8, V).to(dev())
    model.vertex_predictor.ensure_point_pool_proj(1024, dev())
    load_arrays(model, arrs)
    model.set_dropout(0.0)
    model.train()
    points, pcounts = pack([torch.from_numpy(c[0]) for c in clouds])
    return gold, model, clouds, points.to(dev()), pcounts, torch.tensor(counts), V, seed


def _check_outputs(out, gold, tol):
    errs = H.out_errs(out, {k: gold["out." + k] for k in OUT_KEYS})
    print("forward (max-abs rel, element-wise):", {k: (f"{a:.1e}", f"{b:.1e}") for k, (a, b) in errs.items()})
    for k, (a, b) in errs.items():
        assert a < tol and b < tol, (k, a, b)
    lens = [len(e) for e in out["edge_indices"]]
    assert lens == gold["out.edge_index_lens"].tolist()
    flat = np.array([ij for e in out["edge_indices"] for ij in e], dtype=np.int64).reshape(-1, 2)
    assert np.array_equal(flat, gold["out.edge_indices_flat"])                   # exact
    assert np.array_equal(out["actual_vertex_counts"].cpu().numpy(), gold["out.actual_vertex_counts"])
    ep = out["edge_probs"].detach().cpu().numpy()
    for s, n in enumerate(lens):
        assert np.all(ep[s, n:] == 0.0)


def _golden_cotangents(out, seed):
    """The per-cloud cotangents of packed.npz ([1, ...] each) as batch tensors; edge_probs zero past each sample's pairs."""
    cot = {k: torch.zeros(out[k].shape) for k in ("vertices", "existence_probabilities", "edge_probs")}
    for b, e in enumerate(out["edge_indices"]):
        shapes = {"vertices": out["vertices"][b:b + 1], "existence_probabilities": out["existence_probabilities"][b:b + 1],
                  "edge_probs": out["edge_probs"][b:b + 1, :len(e)]}
        for k, v in packed_cotangents(b, shapes, seed).items():
            cot[k][b:b + 1, ..., :v.shape[-1]] = v
    return cot


@pytest.mark.parametrize("mode", FORCED, indirect=True, ids=lambda m: m[0])
def test_forward_packed_vs_golden(mode):
    gold, model, clouds, points, pcounts, counts, V, seed = build_packed()
    out = model.forward_packed(points, pcounts, counts.to(dev()))
    assert list(out.keys()) == ["vertices", "existence_probabilities", "edge_probs", "edge_indices",
                                "global_features", "actual_vertex_counts"]
    _check_outputs(out, gold, TOL_BF16_FWD if mode == "bf16" else TOL_OUT)
    cot = _golden_cotangents(out, seed)
    loss = sum((out[k] * cot[k].to(dev())).sum() for k in cot)
    loss.backward()
    ltol = TOL_BF16_FWD if mode == "bf16" else 1e-4
    assert abs(loss.item() - float(gold["out.loss"])) < ltol * max(1.0, abs(float(gold["out.loss"])))
    named = [(n, p.grad) for n, p in model.named_parameters()]
    bad = H.check_grad_summaries(gold, named, TOL_BF16_GRAD if mode == "bf16" else TOL_GRAD)
    assert not bad, bad
    assert sum(g is not None for _, g in named) == 76


@pytest.mark.parametrize("mode", FORCED[:2], indirect=True, ids=lambda m: m[0])
def test_eval_mode_and_padded_edge_layout(mode):
    """Eval mode (data-dependent counts) is the reference per cloud in eval mode, here: the oracle; the padded edge layout gives
    the ragged outputs in its first edge_width columns, in train and eval mode."""
    gold, model, clouds, points, pcounts, counts, V, seed = build_packed()
    P = oracle.params_from_module(model, requires_grad=False)
    model.eval()
    with torch.no_grad():
        out = model.forward_packed(points, torch.tensor(pcounts))              # a CPU int tensor of counts
        for b, x in enumerate(clouds):
            ref = oracle.model_forward(P, torch.from_numpy(x), None, V, training=False)
            e = ref["edge_probs"].shape[1]
            got = {k: out[k][b:b + 1] for k in OUT_KEYS}
            got["edge_probs"] = out["edge_probs"][b:b + 1, :e]
            for k, (a, c) in H.out_errs(got, ref).items():
                assert a < TOL_OUT and c < TOL_OUT, (b, k, a, c)
            assert out["edge_indices"][b] == ref["edge_indices"][0]
            assert float(out["edge_probs"][b, e:].abs().sum()) == 0.0
        for train in (False, True):
            model.train(train)
            tc = counts.to(dev()) if train else None
            ragged = model.set_edge_layout("ragged").forward_packed(points, pcounts, tc)
            padded = model.set_edge_layout("padded", tail="skip").forward_packed(points, pcounts, tc)
            w = int(padded["edge_width"])
            assert w == ragged["edge_probs"].shape[1]
            assert torch.equal(padded["edge_probs"][:, :w], ragged["edge_probs"])
            assert float(padded["edge_probs"][:, w:].abs().sum()) == 0.0
            assert padded["edge_indices"] == ragged["edge_indices"]
            for k in ("vertices", "existence_probabilities", "global_features"):
                assert torch.equal(padded[k], ragged[k]), k
    model.set_edge_layout("ragged")


# ---------------------------------------------------------------------------------------------------------------------
# decision-frozen gradients: every element of every parameter gradient
# ---------------------------------------------------------------------------------------------------------------------
def _run_frozen(precision, pcounts, V, vcounts, min_rows, kernel_masks, draws):
    from wf3d import config, ops
    from wf3d.packed import pack
    from models.PointCloudToWireframe import PointCloudToWireframe
    old = (config.precision(), config.SPLIT_MIN_ROWS)
    config.set_precision(precision)
    if min_rows is not None:
        config.SPLIT_MIN_ROWS = min_rows
    try:
        torch.manual_seed(20)
        model = PointCloudToWireframe(8, V).to(dev()).set_dropout(0.0)
        model.train()
        with torch.no_grad():
            for n, p in model.named_parameters():
                if p.dim() == 1:
                    p.add_(0.05 * torch.randn(p.shape, generator=torch.Generator().manual_seed(len(n))).to(dev()))
        lay = ops.PackedLayout(pcounts)
        off = lay.offsets.tolist()
        cnt = torch.tensor(vcounts)
        for seed in range(100, 100 + draws):
            gen = torch.Generator().manual_seed(seed)
            clouds = [torch.randn(n, 8, generator=gen) for n in pcounts]
            clouds[0][pcounts[0] - pcounts[0] // 4:] = 0.0          # zero tail in cloud 0
            points, pc = pack(clouds)
            model.zero_grad(set_to_none=True)
            out = model.forward_packed(points.to(dev()), pc, cnt.to(dev()))
            frozen, n_border = H.capture_decisions(out, model, kernel_masks=kernel_masks)
            if n_border == 0:
                break
        else:
            pytest.fail(f"no borderline-free input found in {draws} draws")
        cot = {k: torch.randn(out[k].shape, generator=gen) for k in ("vertices", "existence_probabilities", "edge_probs")}
        sum((out[k] * cot[k].to(dev())).sum() for k in cot).backward()
        got = {n: p.grad.detach().cpu().numpy() for n, p in model.named_parameters() if p.grad is not None}
        P = oracle.params_from_module(model, dtype=torch.float64)
        fwd = {}
        for b, x in enumerate(clouds):
            fz = {"relu": {}, "argmax": {k: v[b:b + 1] for k, v in frozen["argmax"].items()}}
            for name, m in frozen["relu"].items():
                if name.startswith("encoder.mlp."):
                    assert m.shape[0] == lay.M_pad, name             # per-point masks cover the padded rows: slice by offsets
                    fz["relu"][name] = m[off[b]:off[b + 1]]
                else:
                    fz["relu"][name] = m[b:b + 1]
            ref = oracle.model_forward(P, x[None].double(), cnt[b:b + 1], V, training=True, frozen=fz)
            e = ref["edge_probs"].shape[1]
            sum((ref[k] * cot[k][b:b + 1, ..., :ref[k].shape[-1]].double()).sum() for k in cot).backward()
            assert out["edge_indices"][b] == ref["edge_indices"][0]
            o_b = {k: out[k][b:b + 1] for k in OUT_KEYS}
            o_b["edge_probs"] = out["edge_probs"][b:b + 1, :e]
            for k, (a, c) in H.out_errs(o_b, ref).items():
                fwd[k] = tuple(max(u, v) for u, v in zip(fwd.get(k, (0.0, 0.0)), (a, c)))
        errs = {}
        for n in P:
            if P[n].grad is None:
                assert n not in got, n
                continue
            errs[n] = H.elem_err(got[n], P[n].grad.numpy())
        return fwd, errs, seed
    finally:
        config.set_precision(old[0])
        config.SPLIT_MIN_ROWS = old[1]


def _report(tag, fwd, errs, seed):
    worst = sorted(((e, n) for n, e in errs.items()), reverse=True)
    print(f"{tag} packed frozen-decision gradients (input seed {seed}): worst element-wise errors",
          [(f"{e:.1e}", n) for e, n in worst[:5]])
    print("forward (max-abs rel, element-wise):", {k: (f"{a:.1e}", f"{b:.1e}") for k, (a, b) in fwd.items()})


def test_frozen_gradients_packed_fp32_elementwise():
    fwd, errs, seed = _run_frozen("fp32", [96, 37, 160], 12, [12, 2, 7], 1, False, 32)
    _report("fp32", fwd, errs, seed)
    for k, (a, b) in fwd.items():
        assert a < TOL and b < TOL, (k, a, b)
    assert len(errs) == 76
    bad = [(n, e) for n, e in errs.items() if not e <= TOL]
    assert not bad, bad


def test_frozen_gradients_packed_bf16x3_split_routes():
    """M = 4,613 rows, M_pad = 4,864: the default SPLIT_MIN_ROWS takes the split routes, the TN wgrad included (the row
    total is a multiple of 256 only because of the padding).  Per-point ReLU decisions are the forward kernels' own."""
    from wf3d import ops
    pcounts = [700, 1300, 2096, 517]
    lay = ops.PackedLayout(pcounts)
    assert (lay.M, lay.M_pad) == (4613, 4864)
    fwd, errs, seed = _run_frozen("bf16x3", pcounts, 12, [12, 4, 9, 2], None, True, 16)
    _report("bf16x3", fwd, errs, seed)
    for k, (a, b) in fwd.items():
        assert a < TOL and b < TOL, (k, a, b)
    assert len(errs) == 76
    bad = [(n, e) for n, e in errs.items() if not e <= TOL_X3]
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------
# packed is not padded; equal lengths are the dense path
# ---------------------------------------------------------------------------------------------------------------------
def test_packed_is_not_zero_padded():
    """The vertex head's pools are not mask-aware: every pad row of a zero-padded batch adds an mlp(0) row to
    its mean and max, so the padded batch's vertices differ from each cloud's own; the encoder's masked pools do not."""
    gold, model, clouds, points, pcounts, counts, V, seed = build_packed()
    nmax = max(pcounts)
    xpad = torch.zeros(len(clouds), nmax, 8)
    for b, c in enumerate(clouds):
        xpad[b, :pcounts[b]] = torch.from_numpy(c[0])
    with torch.no_grad():
        packed = model.forward_packed(points, pcounts, counts.to(dev()))
        padded = model(xpad.to(dev()), counts.to(dev()))
    errs = H.out_errs(padded, packed, keys=("vertices", "global_features"))
    print("zero-padded vs packed:", errs)
    assert max(errs["vertices"]) > TOL_OUT
    assert max(errs["global_features"]) < TOL_OUT
    b = int(np.argmax(pcounts))                                   # the longest cloud has no pad rows: its own result
    assert H.rel_err(padded["vertices"][b].cpu().numpy(), packed["vertices"][b].cpu().numpy()) < TOL_OUT


@pytest.mark.parametrize("mode", [("fp32", 1), ("bf16x3", 1), ("bf16x3", None)], indirect=True, ids=lambda m: f"{m[0]}-{m[1]}")
def test_equal_lengths_match_the_dense_path(mode):
    from models.PointCloudToWireframe import PointCloudToWireframe
    from wf3d.functional import EncoderFn, EncoderFnPacked
    from wf3d import ops
    B, N, V = 4, 1024, 8                                          # B*N = 4096: a multiple of 256, and >= SPLIT_MIN_ROWS
    torch.manual_seed(3)
    model = PointCloudToWireframe(8, V).to(dev()).set_dropout(0.0)
    model.train()
    x = torch.randn(B, N, 8, device=dev())
    x[1, 900:] = 0.0
    counts = torch.tensor([8, 3, 5, 2], device=dev())
    enc = model.encoder
    args = (enc._n_hidden, mode, *enc._mlp_params())
    lay = ops.PackedLayout.get([N] * B, dev())
    assert lay.M_pad == B * N
    pd, fd, ud = EncoderFn.apply(x, *args)
    pp, fp, up = EncoderFnPacked.apply(x.view(B * N, 8), lay, *args)
    C = fd.shape[-1]
    assert torch.equal(fp, fd.view(B * N, C))                                       # point_features: bit-identical
    assert torch.equal(pp[:, :C], pd[:, :C]) and torch.equal(up[:, C:], ud[:, C:])  # maxima: exact
    sd, sp = pd.grad_fn.saved, pp.grad_fn.saved
    assert torch.equal(sp[5], sd[5]) and torch.equal(sp[6], sd[6]) and torch.equal(sp[7], sd[7])   # arg-max rows, cnt
    dense = model(x, counts)
    packed = model.forward_packed(x.view(B * N, 8), [N] * B, counts)
    for k, (a, b) in H.out_errs(packed, dense).items():
        assert a < TOL_OUT and b < TOL_OUT, (k, a, b)
    assert packed["edge_indices"] == dense["edge_indices"]


# ---------------------------------------------------------------------------------------------------------------------
# capture, host reads, errors
# ---------------------------------------------------------------------------------------------------------------------
def _small():
    from models.PointCloudToWireframe import PointCloudToWireframe
    torch.manual_seed(0)
    m = PointCloudToWireframe(8, 6).to(dev())
    m.vertex_predictor.ensure_point_pool_proj(1024, dev())
    m.set_dropout(0.0)
    m.train()
    pcounts = [300, 41, 130]
    x = torch.randn(sum(pcounts), 8, device=dev())
    return m, x, pcounts, torch.tensor([6, 2, 4], device=dev())


def _loss(o):
    return o["vertices"].sum() + o["existence_probabilities"].sum() + o["edge_probs"].sum()


@pytest.mark.parametrize("mode", [("bf16x3", 1)], indirect=True, ids=lambda m: m[0])
def test_captured_packed_step_replays_equal_eager(mode):
    """forward_packed + backward with fixed point counts, captured with torch.cuda.graph, replays to the eager gradients bit
    for bit (nothing in the packed path syncs; the layout of these counts was uploaded by the warm-up)."""
    m, x, pcounts, c = _small()

    def step():
        for p in m.parameters():
            p.grad = None
        _loss(m.forward_packed(x, pcounts, c)).backward()

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
    assert set(grads) == set(eager) and len(eager) == 76
    for n in eager:
        assert torch.equal(grads[n], eager[n]), n
    for p in m.parameters():
        p.grad = None
    # the graph holds the layout's device addresses: the cache keeps it however many other lists of counts follow
    from wf3d import ops
    lay = ops.PackedLayout.get(pcounts, x.device)
    assert lay.captured
    for n in range(ops.PackedLayout._cache_max + 8):
        ops.PackedLayout.get([n + 1, 3], x.device)
    assert ops.PackedLayout.get(pcounts, x.device) is lay
    assert len(ops.PackedLayout._cache) <= ops.PackedLayout._cache_max + 1 + sum(v.captured for v in ops.PackedLayout._cache.values())
    g.replay()
    torch.cuda.synchronize()
    for n in eager:
        assert torch.equal(grads[n], eager[n]), n
    # a layout is not built inside a capture: its upload would come from a staging buffer that does not outlive it
    g2 = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="warm-up"):
        with torch.cuda.graph(g2):
            ops.PackedLayout.get([5, 6, 7, 8, 9], x.device)


def test_forward_packed_reads_nothing_back():
    """Host point counts and the padded edge layout: no device -> host read in forward_packed, the first call with a new
    list of counts (which uploads their layout) included."""
    m, x, pcounts, c = _small()
    m.set_edge_layout("padded")
    m.forward_packed(x, pcounts, c)                               # warm-up: lazily created state of the other stages
    fresh = [299, 42, 130]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = m.forward_packed(x, fresh, c)
        out2 = m.forward_packed(x, fresh, c)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(out["vertices"], out2["vertices"])
    # a CUDA count tensor is read once, then served from the cache while it is unmodified
    pc = torch.tensor(pcounts, device=dev())
    m.forward_packed(x, pc, c)
    torch.cuda.set_sync_debug_mode("error")
    try:
        m.forward_packed(x, pc, c)
    finally:
        torch.cuda.set_sync_debug_mode("default")


def test_errors_are_raised_on_the_host():
    m, x, pcounts, c = _small()
    with pytest.raises(ValueError, match="sum to"):
        m.forward_packed(x, [300, 41, 129], c)
    with pytest.raises(ValueError, match="at least one point"):
        m.forward_packed(x, [300, 171, 0], c)
    with pytest.raises(ValueError, match="at least one cloud"):
        m.forward_packed(x[:0], [], c)
    with pytest.raises(ValueError, match="contiguous"):
        m.forward_packed(torch.randn(8, sum(pcounts), device=dev()).t(), pcounts, c)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.forward_packed(x.cpu(), pcounts, c)
    with pytest.raises(RuntimeError, match="requires grad"):
        m.forward_packed(x.clone().requires_grad_(), pcounts, c)
    with pytest.raises(ValueError):
        m.forward_packed(x.view(1, -1, 8), pcounts, c)
    # an all-zero cloud behaves as a dead cloud of the dense path: finite outputs, masked pools 0
    z = x.clone()
    z[300:341] = 0.0
    out = m.forward_packed(z, pcounts, c)
    dense = m(z[300:341][None], c[1:2])
    for k, (a, b) in H.out_errs({k: out[k][1:2, ..., :dense[k].shape[-1]] for k in OUT_KEYS}, dense).items():
        assert a < TOL_OUT and b < TOL_OUT, (k, a, b)
    _loss(out).backward()
    assert all(torch.isfinite(p.grad).all() for p in m.parameters() if p.grad is not None)
