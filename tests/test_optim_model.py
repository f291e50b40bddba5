"""tests/optim_model.py on the CPU: (1) clip_adam_step64 against torch's own clip_grad_norm_ + Adam run in float64,
so that the model is pinned to the reference's semantics and not to this project's kernel; (2) compare_step, at its
bounds and on the inputs of the GPU test's hyper-parameter cases, rejects a list of subtly wrong Adam updates;
(3) TrainMeter.read()'s ring logic on a record written by hand."""
import math

import numpy as np
import pytest
import torch

import helpers as H  # noqa: F401  (puts the package on sys.path)
import optim_model as OM


# ---------------------------------------------------------------------------------------------------------------------
# 1. the model against torch in float64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", sorted(OM.HYPER))
def test_model_matches_torch_clip_and_adam_in_float64(row):
    """Five steps of clip_grad_norm_ + Adam(foreach=False) on float64 CPU tensors, with a clip-only tensor (in the norm
    and scaled, not in the optimizer) and, at the third step, one +inf gradient element: every p, g, m, v and the norm
    within 1e-12 (element-wise, of max(|x|, rms)), NaN exactly where torch puts it.  max_norm None and 0.0 both mean
    "no clipping" for ClipAdam, so torch's clip is left out there."""
    hp = OM.HYPER[row]
    rng = np.random.RandomState(7)
    sizes = [33, 200, 7]
    p = [0.02 * rng.standard_normal(n) for n in sizes]
    m = [np.zeros(n) for n in sizes] + [None]
    v = [np.zeros(n) for n in sizes] + [None]
    tp = [torch.nn.Parameter(torch.from_numpy(x.copy())) for x in p]
    lazy = torch.nn.Parameter(torch.zeros(50, dtype=torch.float64))
    opt = torch.optim.Adam(tp, lr=hp["lr"], betas=hp["betas"], eps=hp["eps"], weight_decay=hp["weight_decay"], foreach=False)
    p = p + [None]
    for step in range(1, 6):
        scale = 3.0 if step % 2 else 0.002                      # total norm about 50 and 0.03: both sides of either max_norm
        g = [scale * rng.standard_normal(n) for n in sizes + [50]]
        if step == 3:
            g[1][17] = math.inf
        for q, x in zip(tp + [lazy], g):
            q.grad = torch.from_numpy(x.copy())
        n_ref = OM.grad_norm64(g)
        if hp["max_norm"]:
            n_ref = float(torch.nn.utils.clip_grad_norm_(tp + [lazy], max_norm=hp["max_norm"]))
        opt.step()
        P, G, M, V, n64 = OM.clip_adam_step64(p, g, m, v, step=step, **hp)
        assert n64 == n_ref or abs(n64 - n_ref) <= 1e-12 * n_ref
        for i, q in enumerate(tp + [lazy]):
            assert OM.elem_err_nf(G[i], q.grad.numpy(), "g") <= 1e-12
            if i == len(tp):
                assert P[i] is None and M[i] is None and V[i] is None
                continue
            st = opt.state[q]
            assert int(st["step"]) == step
            assert OM.elem_err_nf(P[i], q.detach().numpy(), "p") <= 1e-12
            assert OM.elem_err_nf(M[i], st["exp_avg"].numpy(), "m") <= 1e-12
            assert OM.elem_err_nf(V[i], st["exp_avg_sq"].numpy(), "v") <= 1e-12
        if step == 3:
            assert n64 == math.inf
            if hp["max_norm"]:                                  # coef 0: inf * 0 = NaN at that element, 0 elsewhere
                assert np.isnan(G[1][17]) and np.count_nonzero(np.nan_to_num(G[1], nan=0.0)) == 0
                assert np.isnan(P[1][17]) and np.isnan(P[1]).sum() == 1
        p, m, v = P, M, V


def test_nan_norm_gives_nan_coefficient_and_no_max_norm_gives_one():
    assert math.isnan(OM.clip_coef64(float("nan"), 1.0))
    assert OM.clip_coef64(float("nan"), None) == 1.0 and OM.clip_coef64(5.0, 0.0) == 1.0 and OM.clip_coef64(5.0, -1.0) == 1.0
    assert OM.clip_coef64(0.25, 1.0) == 1.0 and OM.clip_coef64(math.inf, 1.0) == 0.0
    assert OM.clip_coef64(4.0, 1.0) == 1.0 / (4.0 + 1e-6)


# ---------------------------------------------------------------------------------------------------------------------
# 2. sensitivity: the GPU test's comparison must reject these
# ---------------------------------------------------------------------------------------------------------------------
def _mutant_step64(mutation, p, g, m, v, *, step, lr, betas, eps, weight_decay, max_norm, norm=None):
    """clip_adam_step64 with one thing wrong (None: nothing, the formulas written a second time)."""
    b1, b2 = betas
    norm64 = OM.grad_norm64(g)
    coef = OM.clip_coef64(norm64 if norm is None else norm, max_norm)
    t = step - 1 if mutation == "bias_correction_at_t_minus_1" else step
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    omb2 = float(np.float32(1.0) - np.float32(b2)) if mutation == "one_minus_beta2_in_fp32" else 1.0 - b2
    wd = 0.0 if mutation == "weight_decay_dropped" else weight_decay
    P, G, M, V = [], [], [], []
    with np.errstate(all="ignore"):
        for pi, gi, mi, vi in zip(p, g, m, v):
            gc = np.asarray(gi, dtype=np.float64) * coef
            G.append(np.asarray(gi, dtype=np.float64) if mutation == "clip_not_stored_in_grad" else gc)
            if mi is None:
                P.append(None); M.append(None); V.append(None)
                continue
            p64, m64, v64 = (np.asarray(x, dtype=np.float64) for x in (pi, mi, vi))
            ge = gc + wd * p64 if wd != 0 else gc
            m2 = OM.lerp64(m64, ge, 1.0 - b1)
            v2 = b2 * v64 + omb2 * ge * ge
            if mutation == "eps_inside_sqrt":
                denom = np.sqrt(v2 / bc2 + eps)
            else:
                denom = np.sqrt(v2) / math.sqrt(bc2) + (0.0 if mutation == "eps_dropped" else eps)
            upd = (np.float64(lr) / bc1) * m2 / denom
            if mutation == "update_scaled_by_1.001":
                upd = upd * 1.001
            P.append(p64 - upd); M.append(m2); V.append(v2)
    return P, G, M, V, norm64


def _store32(x):
    with np.errstate(all="ignore"):
        return [None if a is None else np.asarray(a, dtype=np.float64).astype(np.float32) for a in x]


def _cases():
    for row in sorted(OM.HYPER):
        for step in OM.STEPS:
            for side in sorted(OM.SIDES):
                yield row, step, side


def _before(row, step, side):
    hp = OM.HYPER[row]
    norm = OM.SIDES[side] * (hp["max_norm"] or 1.0)
    seed = 1000 * sorted(OM.HYPER).index(row) + 10 * OM.STEPS.index(step) + sorted(OM.SIDES).index(side)
    return OM.make_inputs(OM.HYPER_SIZES, OM.HYPER_CLIP_ONLY, seed=seed, step=step, norm=norm, max_norm=hp["max_norm"])


def _rejected(mutation, row, step, side):
    """Does compare_step refuse the mutant's step, stored as fp32 the way a kernel would store it?"""
    hp = OM.HYPER[row]
    before = _before(row, step, side)
    P, G, M, V, n64 = _mutant_step64(mutation, before["p"], before["g"], before["m"], before["v"], step=step, **hp)
    after = dict(p=_store32(P), g=_store32(G), m=_store32(M), v=_store32(V))
    if mutation == "clip_not_stored_in_grad":
        after["g"] = [x.copy() for x in before["g"]]            # bit for bit the input
    try:
        OM.compare_step(before, after, np.float32(n64), step=step, **hp)
    except AssertionError:
        return True
    return False


def test_comparison_accepts_the_model_stored_in_fp32():
    """The bounds are not so tight that a correctly rounded result misses them: the true model, rounded once to fp32,
    passes every hyper-parameter case; and the second writing of the formulas above is the model when nothing is mutated."""
    for row, step, side in _cases():
        assert not _rejected(None, row, step, side), (row, step, side)
    before = _before("moved", 2, "clipped")
    a = OM.clip_adam_step64(before["p"], before["g"], before["m"], before["v"], step=2, **OM.HYPER["moved"])
    b = _mutant_step64(None, before["p"], before["g"], before["m"], before["v"], step=2, **OM.HYPER["moved"])
    for x, y in zip(a[:4], b[:4]):
        for xi, yi in zip(x, y):
            assert (xi is None and yi is None) or np.array_equal(xi, yi)


# mutation -> cases (row, step, side) that must reject it.  Elsewhere a mutation may be invisible for a good reason:
# eps = 1e-8 is 3e-6 of sqrt(v) here, weight decay 1e-6 changes the gradient by 1e-5, an unclipped step has coef 1, the
# bias corrections at t - 1 = 999 differ by 1e-3 of 0.37 only in the second one, 1 - 0.9 has no fp32 cancellation, and
# once v holds a history, 5e-5 of the (1 - beta2) = 1e-3 share that a step adds is 5e-8 of v.
MUTATIONS = {
    "weight_decay_dropped": [("moved", s, side) for s in OM.STEPS for side in OM.SIDES] + [("defaults", 1, "unclipped")],
    "eps_dropped": [("moved", s, side) for s in OM.STEPS for side in OM.SIDES],
    "eps_inside_sqrt": [("moved", s, side) for s in OM.STEPS for side in OM.SIDES] + [("defaults", 1, "unclipped")],
    "update_scaled_by_1.001": [(r, s, side) for r in OM.HYPER if r != "lr0" for s in OM.STEPS for side in OM.SIDES],
    "bias_correction_at_t_minus_1": [(r, s, side) for r in ("defaults", "moved", "nowd_noclip") for s in OM.STEPS for side in OM.SIDES
                                     if (r, s) != ("moved", 1000)],                 # 1 - 0.9 ** 999 is 1 in float64
    "one_minus_beta2_in_fp32": [(r, 1, side) for r in ("defaults", "lr0", "nowd_noclip", "nowd_max0") for side in OM.SIDES],
    "clip_not_stored_in_grad": [(r, s, "clipped") for r in ("defaults", "moved", "zero_betas", "lr0") for s in OM.STEPS],
}


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_comparison_rejects_a_subtly_wrong_update(mutation):
    missed = [c for c in MUTATIONS[mutation] if not _rejected(mutation, *c)]
    assert not missed, (mutation, missed)
    n = sum(_rejected(mutation, *c) for c in _cases())
    print(f"{mutation}: rejected in {n} of {len(list(_cases()))} cases")
    assert n >= len(MUTATIONS[mutation])


def test_comparison_refuses_a_case_near_the_clip_threshold():
    before = OM.make_inputs([100], [], seed=1, step=1, norm=1.5, max_norm=1.0)
    with pytest.raises(ValueError, match="threshold"):
        OM.compare_step(before, before, np.float32(1.5), step=1, **OM.HYPER["defaults"])


# ---------------------------------------------------------------------------------------------------------------------
# 3. TrainMeter.read() on a record written by hand (no kernel)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity,steps", [(4, 0), (4, 3), (4, 4), (4, 5), (4, 9), (4, 4099), (1, 0), (1, 1), (1, 2), (1, 5),
                                            (0, 0), (0, 1), (0, 5)])
def test_meter_read_returns_the_ring_oldest_first(capacity, steps):
    """steps <, = and > capacity, capacity 1, and capacity 0 (history=0: the kernel keeps no ring; read() used to divide
    by zero after the first update)."""
    from wf3d.meter import TrainMeter
    meter = TrainMeter(torch.device("cpu"), history=capacity)
    assert meter.state.shape == (8 + capacity,)
    meter.state[0] = steps
    meter.state[1:8] = torch.tensor([0.5, 0.25, 1.5, 2.5, 3.5, 4.5, 5.5])
    for t in range(max(0, steps - 2 * capacity - 1), steps):   # as the kernel writes it: step t at 8 + t % capacity
        if capacity:
            meter.state[8 + t % capacity] = 10.0 + t
    m = meter.read()
    assert m["loss_history"] == [10.0 + t for t in range(max(0, steps - capacity), steps)]
    assert m["steps"] == steps
    assert (m["best_loss"], m["best_vertex_rmse"], m["total_loss"], m["vertex_loss"], m["existence_loss"], m["edge_loss"],
            m["vertex_rmse"]) == (0.5, 0.25, 1.5, 2.5, 3.5, 4.5, 5.5)


def test_meter_rejects_a_negative_history():
    from wf3d.meter import TrainMeter
    with pytest.raises(ValueError, match="history"):
        TrainMeter(torch.device("cpu"), history=-1)


# ---------------------------------------------------------------------------------------------------------------------
# meter64 against the reference loop's host formulas (train.py:145-157)
# ---------------------------------------------------------------------------------------------------------------------
def test_meter64_follows_the_host_formulas_and_fminf():
    rng = np.random.RandomState(5)
    tgt = rng.standard_normal((9, 3))
    cap = 4
    s = np.zeros(8 + cap)
    hist, rmses = [], []
    for step in range(7):
        pred = rng.standard_normal((12, 3))
        tot = float("nan") if step in (0, 3) else float(3.0 - 0.3 * step + rng.random_sample())
        s = OM.meter64(s, cap, tot, 1.0 + step, None, 2.0 + step, pred, tgt, count0=7)
        hist.append(tot)
        rmses.append(math.sqrt(np.mean((pred[:7] - tgt[:7]) ** 2)))
        assert s[0] == step + 1 and (s[3] == tot or (tot != tot and s[3] != s[3]))
        assert (s[4], s[5], s[6]) == (1.0 + step, 0.0, 2.0 + step)
        assert abs(s[7] - rmses[-1]) <= 1e-15 and abs(s[2] - min(rmses)) <= 1e-15
        finite = [x for x in hist[1:] if x == x]               # step 0's NaN is replaced by the first number (fminf)
        assert (s[1] != s[1]) if not finite else s[1] == min(finite)
    assert np.array_equal(s[8:], np.array([hist[4], hist[5], hist[6], hist[3]]), equal_nan=True)
    # the clamp, no counts, no vertices
    assert OM.meter64(np.zeros(8), 0, 1.0, None, None, None, pred, tgt, count0=300)[7] == OM.meter64(np.zeros(8), 0, 1.0, None, None, None, pred, tgt)[7]
    assert abs(OM.meter64(np.zeros(8), 0, 1.0, None, None, None, pred, tgt)[7] - math.sqrt(np.mean((pred[:9] - tgt) ** 2))) <= 1e-15
    assert OM.meter64(np.zeros(8), 0, 1.0, None, None, None, pred, tgt, count0=0)[7] == 0.0
    assert OM.meter64(np.zeros(8), 0, 1.0, None, None, None, pred, tgt, count0=-3)[7] == 0.0
