"""Diagnostic: where do the largest edge_mlp.4.weight gradient errors of tests/test_bench_configs_gpu.py come from?

    python scripts/debug_edge_wgrad_outliers.py [case ...]      case = cfg2 | cfg4 | cfg5 | cfg2r | cfg5r | cfg1 (r: ragged)

For each case the bench-configs test is run as the test runs it.  The oracle's edge_mlp.4 operands are recorded on the
way (its input h1 and the gradient dz2 at its output, fp64), and so is the HIP wgrad's own operand pair whenever it runs
on the TN kernel (the sx8 operands unpacked to hi + lo).  Printed per case:

  * the element-wise error map of dW = dz2^T h1: worst elem_err, quantiles of |g - g64| / rms, how many elements exceed
    1e-4, the rows / columns of the 12 worst, and how far the worst row / column rms error stands above the median
    (a kernel bug concentrates in tiles or whole rows / columns; rounding does not);
  * the conditioning of the product, kappa_ij = sum_e |dz2_ei| |h1_ej| / max(|g64_ij|, rms g64): how much larger than the
    element's yardstick the sum of the absolute terms is;
  * err / (u kappa) with u = 2^-17, the relative error of one bf16x3 operand: the observed error in units of the
    rounding the product's own terms can carry.  O(1) at every case means one mechanism; a bug shows as a large value;
  * with the TN operands: the error of the wgrad kernel itself (HIP dW against fp64 of its own operands), and how far
    those operands lie from the oracle's (relative rms error of dz2 and h1 per column).
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import helpers as H  # noqa: E402
import test_bench_configs_gpu as T  # noqa: E402
from oracle import reference_cpu as R  # noqa: E402
from wf3d import ops  # noqa: E402

NAME = "edge_predictor.edge_mlp.4"
U = 2.0 ** -17
CASES = {"cfg1": ("cfg1", False), "cfg2": ("cfg2", False), "cfg4": ("cfg4", False), "cfg5": ("cfg5", False),
         "cfg2r": ("cfg2", True), "cfg5r": ("cfg5", True)}


def run(case):
    cfg, ragged = CASES[case]
    rec = {"h1": [], "z2": [], "tn": None}
    lin0, elem0, tn0, routes0 = R._lin, H.elem_err, ops.gemm_split_tn, T.check_routes

    def lin(P, name, x):
        y = lin0(P, name, x)
        if name == NAME and y.requires_grad:
            y.retain_grad()
            rec["h1"].append(x.detach())
            rec["z2"].append(y)
        return y

    def elem(a, b, floor=None):
        if np.shape(a) == (256, 512):
            rec["g"], rec["g64"] = np.asarray(a, np.float64), np.asarray(b, np.float64)
        return elem0(a, b, floor)

    def tn(a_s, b_s, *a, **k):
        out = tn0(a_s, b_s, *a, **k)
        if {a_s.shape[1], b_s.shape[1]} == {256, 512} and a_s.shape[0] != a_s.shape[1]:
            to = lambda t: sum(H.unpack_sx8(t)).double()                               # noqa: E731
            dz, h = (a_s, b_s) if a_s.shape[1] == 256 else (b_s, a_s)
            rec["tn"] = (to(dz), to(h))
        return out

    R._lin, H.elem_err, ops.gemm_split_tn, T.check_routes = lin, elem, tn, (lambda *a, **k: None)
    try:
        T.run_config([], cfg, "bf16x3", ragged=ragged)
    finally:
        R._lin, H.elem_err, ops.gemm_split_tn, T.check_routes = lin0, elem0, tn0, routes0
    g, g64 = rec["g"], rec["g64"]
    h1 = torch.cat(rec["h1"])
    dz2 = torch.cat([z.grad for z in rec["z2"]])
    del rec["z2"]
    rms = np.sqrt(np.mean(g64 * g64))
    yard = np.maximum(np.abs(g64), rms)
    e = np.abs(g - g64) / yard
    d = np.abs(g - g64) / rms
    kappa = (dz2.abs().T @ h1.abs()).cpu().numpy() / yard
    r = e / (U * kappa)
    worst = np.argsort(e.ravel())[::-1][:12]
    rows, cols = np.unravel_index(worst, e.shape)
    rr, cc = np.sqrt(np.mean(d * d, axis=1)), np.sqrt(np.mean(d * d, axis=0))
    i = worst[0]
    print(f"[{case}] {h1.shape[0]} edge rows: worst elem_err {e.max():.2e} at {np.unravel_index(i, e.shape)}; "
          f"|g-g64|/rms quantiles 50/99/99.9/max {np.quantile(d, .5):.1e} {np.quantile(d, .99):.1e} "
          f"{np.quantile(d, .999):.1e} {d.max():.1e}; n > 1e-4: {int((e > 1e-4).sum())}/{e.size}; "
          f"L2 {np.linalg.norm(g - g64) / np.linalg.norm(g64):.1e}")
    print(f"[{case}]   worst rows {rows.tolist()} cols {cols.tolist()}; row-rms max/median {rr.max() / np.median(rr):.1f}, "
          f"col-rms max/median {cc.max() / np.median(cc):.1f}")
    print(f"[{case}]   kappa: median {np.median(kappa):.0f}, at the worst element {kappa.ravel()[i]:.0f}, max {kappa.max():.0f}; "
          f"err/(u kappa): at the worst element {r.ravel()[i]:.2f}, max {r.max():.2f}, median {np.median(r):.3f}")
    if rec["tn"] is not None:
        dz_k, h_k = rec["tn"]
        own = (dz_k.T @ h_k).cpu().numpy()
        ek = np.abs(g - own) / yard
        col_err = lambda a, b: ((a - b).norm(dim=0) / b.norm(dim=0).clamp_min(1e-300)).max().item()   # noqa: E731
        eo = np.abs(own - g64) / yard
        print(f"[{case}]   wgrad kernel vs fp64 of its own operands: worst {ek.max():.2e}; its operands' product vs "
              f"oracle: worst {eo.max():.2e}; operand column rel-rms error: dz2 {col_err(dz_k, dz2):.1e}, "
              f"h1 {col_err(h_k, h1):.1e}")
        # which operand carries it: the kernel's dz2 with the oracle's h1, and the other way round
        e_dz = np.abs((dz_k.T @ h1).cpu().numpy() - g64) / yard
        e_h = np.abs((dz2.T @ h_k).cpu().numpy() - g64) / yard
        print(f"[{case}]   worst with only dz2 from the kernel {e_dz.max():.2e}, with only h1 from the kernel {e_h.max():.2e}")
    T.free()


if __name__ == "__main__":
    for c in sys.argv[1:] or ["cfg2", "cfg4", "cfg2r", "cfg5"]:
        run(c)
