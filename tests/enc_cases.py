"""Shared by tests/test_encoder_cotangents_gpu.py and tests/test_enc_cases.py: the fp64 reference of the encoder alone
(dense and packed, decision-frozen or not), the inputs, and the driver that runs PointNetEncoder.encode / encode_packed
against it.

The reference is oracle/reference_cpu.py's: encoder_forward(P, x, frozen=...) gives (g, point_features), and
upooled = [unmasked mean | unmasked max] is formed from point_features as vertex_forward forms it.  A packed batch is
that, cloud by cloud, on [1, n_b, D]."""
import itertools

import numpy as np
import torch

import helpers as H
from helpers import oracle

OUTS = ("g", "pf", "up")                     # (global, point_features, upooled), the order encode() returns them in
SUBSETS = [s for k in (1, 2, 3) for s in itertools.combinations(OUTS, k)]      # the 7 non-empty subsets
PF_COT_SCALE = 0.01                          # as tests/test_model_gpu.py::test_encoder_other_widths_vs_oracle


# ----------------------------------------------------------------------------------------------------------------------
# fp64 reference
# ----------------------------------------------------------------------------------------------------------------------
def ref_dense(P, x, frozen=None):
    """(g [B, C], point_features [B, N, C], upooled [B, 2C]) of x [B, N, D]; P keyed "encoder. ..."."""
    g, pf = oracle.encoder_forward(P, x, frozen=frozen)
    if frozen is not None:
        umax = oracle._max_over_points(pf, frozen, "vert_unmasked")
    else:
        umax = pf.max(dim=1).values
    return g, pf, torch.cat([pf.mean(dim=1), umax], dim=1)


def own_decisions(P, x):
    """The decisions ref_dense(P, x) takes itself, in the form `frozen` has: ReLU masks [B*N, width] / [B, width], arg-max
    rows [B, C] (-1: a cloud without a valid point)."""
    relu = {}

    def block(h, lin, ln):
        v = oracle._ln(P, ln, oracle._lin(P, lin, h))
        relu[ln] = v > 0
        return torch.relu(v)

    with torch.no_grad():
        B, N, D = x.shape
        n_lin = oracle._count_blocks(P, "encoder.mlp.", 4)
        h = x.reshape(B * N, D)
        for i in range(n_lin - 1):
            h = block(h, f"encoder.mlp.{4 * i}", f"encoder.mlp.{4 * i + 1}")
        pf = oracle._lin(P, f"encoder.mlp.{4 * (n_lin - 1)}", h).reshape(B, N, -1)
        valid = x.abs().sum(-1) > 1e-9
        mv, mi = torch.where(valid.unsqueeze(-1), pf, torch.full_like(pf, float("-inf"))).max(dim=1)
        arg_m = torch.where(torch.isfinite(mv), mi, torch.full_like(mi, -1))
        mx = torch.where(torch.isfinite(mv), mv, torch.zeros_like(mv))
        avg = (pf * valid.unsqueeze(-1)).sum(1) / valid.sum(1, keepdim=True).clamp(min=1).to(pf.dtype)
        h = block(torch.cat([mx, avg], 1), "encoder.feature_fusion.0", "encoder.feature_fusion.1")
        block(h, "encoder.feature_fusion.3", "encoder.feature_fusion.4")
        return {"relu": relu, "argmax": {"enc_masked": arg_m, "vert_unmasked": pf.max(dim=1).indices}}


def slice_frozen(frozen, b, r0, r1):
    """Cloud b's part of a packed batch's per-point decisions: the masks of rows r0 .. r1-1, the arg-max rows of cloud b."""
    if frozen is None:
        return None
    relu = {k: m[r0:r1] for k, m in frozen["relu"].items() if ".mlp." in k}
    return {"relu": relu, "argmax": {k: a[b:b + 1] for k, a in frozen["argmax"].items()}}


def ref_packed(P, pts, counts, frozen=None):
    """The same of a packed batch pts [M, D] with M = sum(counts): (g [B, C], point_features [M, C], upooled [B, 2C]).  The
    per-point MLP and the pools are the oracle's on each cloud alone, as [1, n_b, D]; the arg-max rows are local to the
    cloud.  A cloud of no rows pools to zeros and contributes no gradient to the per-point MLP.  The fusion MLP then runs
    once over the [B, 2C] pooled vectors, as it does in the dense reference (row by row it would be the same function
    through another BLAS routine, and g would differ from the dense reference's in the last bit)."""
    C = P[f"encoder.mlp.{4 * (oracle._count_blocks(P, 'encoder.mlp.', 4) - 1)}.weight"].shape[0]
    pooled, pfs, ups, r0 = [], [], [], 0
    for b, n in enumerate(counts):
        if n == 0:
            pooled.append(pts.new_zeros(1, 2 * C)), ups.append(pts.new_zeros(1, 2 * C))
            continue
        x = pts[r0:r0 + n].unsqueeze(0)
        fz = slice_frozen(frozen, b, r0, r0 + n)
        pf = oracle.encoder_point_mlp(P, x[0], frozen=fz).unsqueeze(0)
        mx, avg = oracle.encoder_pools(x, pf, fz)
        umax = pf.max(dim=1).values if fz is None else oracle._max_over_points(pf, fz, "vert_unmasked")
        pooled.append(torch.cat([mx, avg], dim=1)), pfs.append(pf[0]), ups.append(torch.cat([pf.mean(dim=1), umax], dim=1))
        r0 += n
    assert r0 == pts.shape[0]
    return oracle.encoder_fusion(P, torch.cat(pooled), frozen=frozen), torch.cat(pfs), torch.cat(ups)


# ----------------------------------------------------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------------------------------------------------
def dense_input(seed, B, N, din=8):
    """Seeded Gaussian clouds as tests/test_frozen_grad_gpu.py draws them: a zero-padded tail in cloud 0 (valid rows
    0 .. N - N // 4 - 1) and, where B >= 2, an all-zero cloud 1."""
    x = torch.randn(B, N, din, generator=torch.Generator().manual_seed(seed))
    x[0, N - N // 4:] = 0.0
    if B >= 2:
        x[1] = 0.0
    return x


def packed_input(seed, counts, din=8):
    """The same packed: clouds of `counts` rows, cloud 0 with a zero tail, cloud 1 (where it has rows) all zero."""
    g = torch.Generator().manual_seed(seed)
    clouds = [torch.randn(n, din, generator=g) for n in counts]
    clouds[0][counts[0] - counts[0] // 4:] = 0.0
    if len(counts) >= 2:
        clouds[1][:] = 0.0
    return torch.cat(clouds)


def cotangents(seed, shapes):
    """Seeded Gaussian cotangents of the three outputs, point_features' scaled by PF_COT_SCALE."""
    g = torch.Generator().manual_seed(seed)
    cot = {k: torch.randn(shapes[k], generator=g) for k in OUTS}
    cot["pf"] *= PF_COT_SCALE
    return cot


def perturb_1d(module):
    """1-D parameters moved by 0.05 so that no LayerNorm affine is the identity and no bias zero."""
    with torch.no_grad():
        for n, p in module.named_parameters():
            if p.dim() == 1:
                p.add_((0.05 * torch.randn(p.shape, generator=torch.Generator().manual_seed(len(n)))).to(p.device))


def backward_subset(outs, cot, subset):
    """Backpropagates sum(out_k * cot_k) over k in subset (the outputs' cotangents handed to autograd directly)."""
    keys = [k for k in OUTS if k in subset]
    torch.autograd.backward([outs[k] for k in keys], [cot[k].to(outs[k].device, outs[k].dtype) for k in keys])


def grad_errors(got, P, prefix="encoder."):
    """{name: H.elem_err} of every parameter gradient; a parameter the outputs do not reach has no gradient on either
    side."""
    errs = {}
    for n, ref in P.items():
        name = n[len(prefix):]
        if ref.grad is None:
            assert got.get(name) is None, f"{name}: a gradient where the reference has none"
            continue
        assert got.get(name) is not None, f"{name}: no gradient where the reference has one"
        errs[name] = H.elem_err(got[name].detach().cpu().numpy(), ref.grad.numpy())
    return errs


def out_errors(outs, ref):
    """{output: (max-abs error on the tensor's scale, element-wise error)} as H.out_errs."""
    res = {}
    for k in OUTS:
        a, b = outs[k].detach().double().cpu().numpy(), ref[k].detach().numpy()
        res[k] = (H.rel_err(a, b), H.elem_err(a, b))
    return res


def params64(encoder):
    P = oracle.params_from_module(encoder, dtype=torch.float64)
    return {"encoder." + k: v for k, v in P.items()}


def np_grads(module):
    return {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in module.named_parameters()}
