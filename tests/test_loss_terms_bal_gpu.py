"""wf3d_loss_terms_assigned_bal (csrc/loss.hip: loss_terms_kernel's balanced / focal edge element) against float64 torch
autograd of the formula it documents,

    L(p, t) = -( w t (1-p)^gamma max(log p, -100) + (1-t) p^gamma max(log1p(-p), -100) ),

averaged over B x the common width, with the vertex and existence terms of tests/test_loss_terms_forms_gpu.py.  The case
generator and the shapes are that file's (a random permutation per sample as the assignment, target width != V in both
directions, V > 256, B > 64, no edge columns, the strided view); here every sample's first two edge columns are
p = t = 0 and p = t = 1, the columns a ragged batch pads with, which must give exactly 0 and gradient exactly 0.  The
float64 reference leaves those columns out of the sum (autograd of log at 0 is 0 / 0) and keeps them in the normaliser.

(w, gamma) in {(1, 0), (4, 0), (1, 2), (3, 0.5)}, without and with a device edge width.  Bounds are that file's: each
loss within 5e-6 x max(1, |ref|), each gradient tensor within 2e-5 of its largest element; gradients of edge columns
past the common width are exactly 0; at (1, 0) the entry returns the bits of wf3d_loss_terms_assigned / _ew."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

WEIGHTS = (3.0, 1.0, 1.5)            # vertex, existence, edge: the kernels' order
# (B, V, Vt, Ep, Et, strided vertices)
SHAPES = [(1, 1, 1, 0, 0, False), (3, 5, 9, 10, 10, False), (3, 9, 5, 36, 20, False), (2, 320, 320, 600, 51040, False),
          (70, 4, 4, 6, 6, False), (4, 12, 12, 66, 66, True)]
IDS = ["B1_V1_noedges", "Vt_wider", "Vt_narrower", "V320", "B70", "strided_view"]
BALANCE = [(1.0, 0.0), (4.0, 0.0), (1.0, 2.0), (3.0, 0.5)]


def dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def case(shape):
    """Inputs of one shape (CPU, float32) and a random permutation per sample."""
    B, V, Vt, Ep, Et, _ = shape
    g = torch.Generator().manual_seed(B * 100003 + V * 101 + Vt)
    top = min(V, Vt)
    counts = torch.randint(0, top + 1, (B,), generator=g)
    counts[0] = top
    if B > 2:
        counts[1] = 0
    c = {"pv": torch.randn(B, V, 3, generator=g) * 1.5,              # |d| on both sides of SmoothL1's beta
         "pe": torch.sigmoid(2.0 * torch.randn(B, V, generator=g)),
         "pp": torch.sigmoid(2.0 * torch.randn(B, Ep, generator=g)),
         "tv": torch.randn(B, Vt, 3, generator=g),
         "te": (torch.arange(V)[None, :] < counts[:, None]).float(),
         "tl": (torch.rand(B, Et, generator=g) > 0.7).float(),
         "counts": counts,
         "c4r": torch.stack([torch.randperm(V, generator=g) for _ in range(B)]).to(torch.int32)}
    if min(Ep, Et) >= 2:
        c["pp"][:, 0], c["tl"][:, 0] = 0.0, 0.0
        c["pp"][:, 1], c["tl"][:, 1] = 1.0, 1.0
    matched = c["c4r"] < counts[:, None]                              # [B, V]
    bs, ps = matched.nonzero(as_tuple=True)
    c["matched"], c["m_b"], c["m_pred"], c["m_tgt"] = matched, bs, ps, c["c4r"][bs, ps].long()
    return c


def edge_element64(p, t, w, gamma):
    lp, lq = torch.log(p).clamp(min=-100.0), torch.log1p(-p).clamp(min=-100.0)
    return -(w * t * (1.0 - p) ** gamma * lp + (1.0 - t) * p ** gamma * lq)


@functools.lru_cache(maxsize=None)
def reference(shape, width, w, gamma):
    """(losses [4], dverts, dexist, dedge, common width) in float64 from autograd; `width` is the prediction's edge width."""
    c = case(shape)
    B, V, Vt, Ep, Et, _ = shape
    pv, pe, pp = (c[k].double().requires_grad_() for k in ("pv", "pe", "pp"))
    n = len(c["m_b"])
    if n:
        lv = torch.nn.functional.smooth_l1_loss(pv[c["m_b"], c["m_pred"]], c["tv"].double()[c["m_b"], c["m_tgt"]],
                                                reduction="sum", beta=1.0) / (3 * n)
    else:
        lv = pv.sum() * 0.0
    le = torch.nn.BCELoss()(pe, c["te"].double())
    cw = min(width, Ep, Et)
    if cw > 0:
        p, t = pp[:, :cw], c["tl"].double()[:, :cw]
        live = ~((p == t) & ((t == 0) | (t == 1)))                   # the p = t columns contribute exactly 0
        ld = edge_element64(p[live], t[live], w, gamma).sum() / (B * cw)
    else:
        ld = pp.sum() * 0.0
    total = WEIGHTS[0] * lv + WEIGHTS[1] * le + WEIGHTS[2] * ld
    total.backward()
    return torch.stack([lv, le, ld, total]).detach(), pv.grad, pe.grad, pp.grad, cw


def run(shape, width, w, gamma, entry="bal"):
    from wf3d import ops
    c = case(shape)
    B, V, Vt, Ep, Et, strided = shape
    d = {k: c[k].to(dev()) for k in ("pe", "pp", "tv", "te", "tl", "counts", "c4r")}
    if strided:                          # what the model passes: the first three columns of its [B, V, 4] output
        out4 = torch.full((B, V, 4), float("nan"))
        out4[:, :, :3] = c["pv"]
        pv = out4.to(dev())[:, :, :3]
        assert not pv.is_contiguous()
    else:
        pv = c["pv"].to(dev())
    ew = None if width is None else torch.tensor(width, dtype=torch.int64, device=dev())
    if entry == "plain":
        return ops.loss_terms_assigned(pv, d["pe"], d["pp"], d["tv"], d["te"], d["tl"], d["c4r"], d["counts"], WEIGHTS,
                                       edge_width=ew)
    return ops.loss_terms_assigned_bal(pv, d["pe"], d["pp"], d["tv"], d["te"], d["tl"], d["c4r"], d["counts"], WEIGHTS,
                                       w, gamma, edge_width=ew)


def check(got, shape, width, w, gamma):
    c = case(shape)
    Ep, Et = shape[3], shape[4]
    ref_l, ref_dv, ref_de, ref_dd, cw = reference(shape, Ep if width is None else width, w, gamma)
    losses, dv, de, dd = (t.cpu().double() for t in got)
    for k, name in enumerate(("vertex", "existence", "edge", "total")):
        err, lim = abs(float(losses[k]) - float(ref_l[k])), 5e-6 * max(1.0, abs(float(ref_l[k])))
        print(f"w {w} gamma {gamma} width {width}: {name} loss {float(losses[k]):.9g} ref {float(ref_l[k]):.9g} err {err:.2e} limit {lim:.2e}")
        assert err < lim, name
    for name, a, b in (("dverts", dv, ref_dv), ("dexist", de, ref_de), ("dedge", dd, ref_dd)):
        assert a.shape == b.shape, name
        if b.numel() == 0:
            continue
        err, lim = float((a - b).abs().max()), 2e-5 * max(float(b.abs().max()), 1e-12)
        print(f"w {w} gamma {gamma} width {width}: {name} max err {err:.2e} limit {lim:.2e}")
        assert err <= lim, name
    assert float(dv[~c["matched"]].abs().sum()) == 0.0                  # unmatched predictions: exactly 0
    assert float(dd[:, cw:].abs().sum()) == 0.0                         # past the common width: exactly 0
    if min(Ep, Et) >= 2:
        assert float(dd[:, :2].abs().sum()) == 0.0                      # p = t = 0 and p = t = 1: exactly 0


def widths(shape):
    Ep = shape[3]
    return [None] + sorted({0, Ep // 2, Ep + 3})


@pytest.mark.parametrize("w, gamma", BALANCE, ids=[f"w{w:g}_g{g:g}" for w, g in BALANCE])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_balanced_terms_against_float64_autograd(shape, w, gamma):
    for width in widths(shape):
        check(run(shape, width, w, gamma), shape, width, w, gamma)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_weight_one_gamma_zero_is_the_plain_entry_bit_for_bit(shape):
    for width in widths(shape):
        for a, b in zip(run(shape, width, 1.0, 0.0), run(shape, width, 1.0, 0.0, entry="plain")):
            assert torch.equal(a, b), width


@pytest.mark.parametrize("gamma", [0.0, 0.5, 1.0, 2.0, 5.0])
def test_columns_that_equal_their_label_give_exact_zeros(gamma):
    """Every edge column p = t in {0, 1}, as in a batch whose samples have no pairs: the edge loss is exactly 0 and no
    edge column gets a gradient, whatever pow makes of 0^gamma and 0^(gamma - 1)."""
    from wf3d import ops
    B, V, E = 3, 5, 10
    g = torch.Generator().manual_seed(5)
    tl = (torch.rand(B, E, generator=g) > 0.5).float().to(dev())
    pv, tv = torch.randn(B, V, 3, generator=g).to(dev()), torch.randn(B, V, 3, generator=g).to(dev())
    pe = torch.sigmoid(torch.randn(B, V, generator=g)).to(dev())
    te = torch.ones(B, V, device=dev())
    c4r = torch.arange(V, dtype=torch.int32, device=dev()).repeat(B, 1)
    counts = torch.full((B,), V, dtype=torch.int64, device=dev())
    losses, _, _, dd = ops.loss_terms_assigned_bal(pv, pe, tl.clone(), tv, te, tl, c4r, counts, WEIGHTS, 4.0, gamma)
    assert float(losses[2]) == 0.0 and float(dd.abs().sum()) == 0.0 and bool(torch.isfinite(losses).all())
