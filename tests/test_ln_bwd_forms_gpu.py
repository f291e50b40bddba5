"""Every branch of the LayerNorm-backward family's one launch routine (csrc/rowops.hip, ln_bwd_launch<KX, PAIR>).

wf3d_ln_act_bwd / _first / _wsum / wf3d_edge_pair_ln_bwd describe their call and one routine picks the kernel
ln_act_bwd_kernel<NS, WPR, KX, PAIR>.  Widths and the (NS, WPR) each selects:

    D = 8 (1,1)   264 (1,2: slices of 136 columns)   520 (1,4)   1032 (2,4)   2056 (4,4: three live slots)   4096 (4,4: full)

with R = 5 (fewer rows than one workgroup pass) and R = 4100 (> 4 * 1024: some workgroups take a second and a fifth
row group).  The first-layer and pair forms stop at 1024 columns: 1032 must be refused by either.

Bounds are the ones of tests/test_kernels_gpu.py: test_ln_act_bwd (fp64 formula; here with the host's dropout mask,
oracle/dropout.py, on the cotangent), test_ln_prep_and_bwd_split_output (the sx8 copy is the exact split of dz),
test_ln_act_bwd_with_weighted_column_sum, test_first_layer_fused_forward_and_backward and
test_pair_ln_backward_without_the_stored_preactivation."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import helpers as H  # noqa: E402,F401  (sets sys.path)
from helpers import unpack_sx8  # noqa: E402
from oracle import dropout as D_  # noqa: E402

TOL_ELT = 2e-5
P, SEED = 0.1, 77
WIDTHS = [8, 264, 520, 1032, 2056, 4096]
ROWS = [5, 4100]


@pytest.fixture(scope="module")
def ops():
    from wf3d import ops as o
    o._lib.load()
    return o


def dev():
    return torch.device("cuda:0")


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    if a.numel() == 0:
        return 0.0
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed + 1000 * len(shape) + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).to(dev())


def ref_split(x):
    hi = x.to(torch.bfloat16).float()
    lo = (x - hi).to(torch.bfloat16).float()
    return hi, lo


def ln_gelu_bwd64(Z, gamma, beta, cot):
    """fp64 gradients of gelu(LayerNorm(Z)) under the cotangent `cot` (the formula of test_ln_act_bwd), on the device."""
    Zc = Z.double().requires_grad_()
    g64, b64 = gamma.double().requires_grad_(), beta.double().requires_grad_()
    y = torch.nn.functional.gelu(torch.nn.functional.layer_norm(Zc, (Z.shape[-1],), g64, b64, 1e-5))
    y.backward(cot)
    return Zc.grad, g64.grad, b64.grad


@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("R", ROWS)
def test_every_width_through_the_plain_wsum_and_first_layer_forms(ops, R, D):
    Z = rnd(R, D, seed=1, scale=1.5) + 0.2
    gamma, beta = 1 + 0.2 * rnd(D, seed=2), 0.1 * rnd(D, seed=3)
    dh = rnd(R, D, seed=4)
    mu, rs = ops.row_stats(Z)

    # 1. wf3d_ln_act_bwd: GELU, dropout, fp32 dz + sx8 dz + the three sums in one [3][D] buffer
    keep = torch.from_numpy(D_.keep(SEED, np.arange(R)[:, None], np.arange(D)[None, :], P)).to(dev())
    cot = dh.double() * keep.double() * float(D_.thresh_scale(P)[1])
    dz64, dg64, db64 = ln_gelu_bwd64(Z, gamma, beta, cot)
    ds = torch.empty_like(Z)
    dz, dg, db, dbias = ops.ln_act_bwd(dh, Z, mu, rs, gamma, beta, ops.ACT_GELU, P, SEED, dz_split=ds)
    e = (rel(dz, dz64), rel(dg, dg64), rel(db, db64), rel(dbias, dz64.sum(0)))
    print(f"R={R} D={D}: ln_act_bwd dz {e[0]:.2e} dgamma {e[1]:.2e} dbeta {e[2]:.2e} dbias {e[3]:.2e}")
    assert e[0] < 5 * TOL_ELT and e[1] < 5 * TOL_ELT and e[2] < 5 * TOL_ELT
    assert e[3] < 2e-4                                     # LN backward rows sum to ~0: compare on dz scale
    hi, lo = unpack_sx8(ds)
    eh, el = ref_split(dz)
    assert torch.equal(hi, eh) and torch.equal(lo, el)     # sx8 copy of dz is the exact split of dz

    # 2. wf3d_ln_act_bwd_wsum on the same inputs
    wrow = rnd(R, seed=5).abs()
    dz2, dg2, db2, wsum = ops.ln_act_bwd_wsum(dh.clone(), Z, wrow, mu, rs, gamma, beta, ops.ACT_GELU, P, SEED)
    e = (rel(dg, dg2), rel(db, db2), rel(wsum, (dz.double() * wrow.double()[:, None]).sum(0)))
    print(f"R={R} D={D}: ln_act_bwd_wsum dgamma {e[0]:.2e} dbeta {e[1]:.2e} wsum {e[2]:.2e}")
    assert torch.equal(dz, dz2) and e[0] < 1e-6 and e[1] < 1e-6
    assert e[2] < 2e-5

    # 3. wf3d_ln_act_bwd_first (ReLU, no dropout, dz not written) against wf3d_ln_act_bwd + the fp64 dz^T x
    if D <= 1024:
        dzr, dgr, dbr, dbiasr = ops.ln_act_bwd(dh, Z, mu, rs, gamma, beta, ops.ACT_RELU)
    for K in (8, 3):
        x = rnd(R, K, seed=6)
        x[::7] = 0.0
        if D > 1024:
            if D == 1032:                                  # the limit survives the shared routine
                with pytest.raises(RuntimeError):
                    ops.ln_act_bwd_first(dh, Z, x, mu, rs, gamma, beta, ops.ACT_RELU)
            continue
        dg1, db1, dbias1, dW = ops.ln_act_bwd_first(dh, Z, x, mu, rs, gamma, beta, ops.ACT_RELU)
        e = (rel(dg1, dgr), rel(db1, dbr), rel(dbias1, dbiasr), rel(dW, dzr.double().T @ x.double()))
        print(f"R={R} D={D} K={K}: ln_act_bwd_first dgamma {e[0]:.2e} dbeta {e[1]:.2e} dbias {e[2]:.2e} dW {e[3]:.2e}")
        assert e[0] < 1e-5 and e[1] < 1e-5 and e[2] < 2e-5
        assert e[3] < 2e-5


@pytest.mark.parametrize("counts", [[9, 2, 5], [40, 2, 17, 33]])
@pytest.mark.parametrize("Hd", [64, 264, 520, 1024, 1032])
def test_every_width_through_the_pair_form(ops, Hd, counts):
    """wf3d_edge_pair_ln_bwd (pre rebuilt in the kernel) against wf3d_ln_act_bwd_wsum on the stored pre: the same kernel
    body on the same floats.  1032 columns: refused."""
    meta = ops.EdgeMeta(counts, dev())
    Pa, Pb = rnd(meta.Rv, Hd, seed=1), rnd(meta.Rv, Hd, seed=2)
    cv = rnd(meta.Rv, 3, seed=3)
    W0 = rnd(Hd, 2 * Hd + 7, seed=4, scale=0.2)
    gamma, beta = 1.0 + 0.1 * rnd(Hd, seed=5), 0.1 * rnd(Hd, seed=6)
    pre, mu, rs, delta = ops.edge_pair_fwd(Pa, Pb, cv, W0, meta)
    dh = rnd(meta.Re, Hd, seed=7)
    if Hd > 1024:
        with pytest.raises(RuntimeError):
            ops.edge_pair_ln_bwd(dh.clone(), Pa, Pb, delta, W0, meta, mu, rs, gamma, beta, ops.ACT_GELU, P, 1234)
        return
    dz, dg, db, wsum = ops.ln_act_bwd_wsum(dh.clone(), pre, delta, mu, rs, gamma, beta, ops.ACT_GELU, P, 1234)
    dz2, dg2, db2, wsum2 = ops.edge_pair_ln_bwd(dh.clone(), Pa, Pb, delta, W0, meta, mu, rs, gamma, beta, ops.ACT_GELU, P, 1234)
    e = (rel(dg2, dg), rel(db2, db), rel(wsum2, wsum))
    print(f"H={Hd} counts={counts}: pair form dgamma {e[0]:.2e} dbeta {e[1]:.2e} wsum {e[2]:.2e}")
    assert torch.equal(dz, dz2)
    assert e[0] < 1e-6 and e[1] < 1e-6 and e[2] < 1e-6


@pytest.mark.parametrize("D", [8, 4096])
def test_no_rows_gives_zero_sums(ops, D):
    """R = 0 passes wf3d_ln_act_bwd (and only it): nothing is launched and the three sums are cleared, as one [3][D]
    buffer and as separate ones."""
    Z, dh = torch.empty(0, D, device=dev()), torch.empty(0, D, device=dev())
    mu, rs = torch.empty(0, device=dev()), torch.empty(0, device=dev())
    gamma, beta = 1 + 0.2 * rnd(D, seed=2), 0.1 * rnd(D, seed=3)
    for kw in ({}, {"want_bias": False}):
        dz, dg, db, dbias = ops.ln_act_bwd(dh, Z, mu, rs, gamma, beta, ops.ACT_GELU, P, SEED, **kw)
        assert dz.shape == (0, D)
        for s in (dg, db, dbias):
            assert s is None or (s.shape == (D,) and not s.any())
        assert (dbias is None) == bool(kw)
