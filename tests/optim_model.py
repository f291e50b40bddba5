"""A numpy model, in float64, of the step tail: torch.nn.utils.clip_grad_norm_ + torch.optim.Adam (csrc/optim.hip,
wf3d.optim.ClipAdam) and of the training meter's record (meter_update_kernel in csrc/loss.hip, wf3d.meter.TrainMeter).

  clip_adam_step64(p, g, m, v, ...)   one step over lists of arrays -> (p', g', m', v', norm64), all float64
  compare_step(before, after, ...)    the comparison of a stored fp32 step with that model, and its bounds
  meter64(state, capacity, ...)       one meter update -> the next record, float64

tests/test_optim_model.py pins clip_adam_step64 to torch's own float64 arithmetic and shows that compare_step, at its
bounds, rejects a list of subtly wrong Adam updates; tests/test_optim_forms_gpu.py and tests/test_meter_forms_gpu.py
hold the kernels to the models."""
import math

import numpy as np

TOL = 2e-6            # helpers.elem_err bound of tests/test_optim_gpu.py, here on g', m', v' and on the UPDATE p' - p
NORM_TOL = 1e-5       # reported norm, relative (tests/test_optim_gpu.py)


def clip_coef64(norm, max_norm):
    """clip_grad_norm_'s coefficient clamp(max_norm / (norm + 1e-6), max=1); a NaN norm stays NaN (torch.clamp keeps it);
    max_norm None or <= 0: no clipping."""
    if max_norm is None or max_norm <= 0:
        return 1.0
    norm = float(norm)
    if norm != norm:
        return float("nan")
    return min(1.0, max_norm / (norm + 1e-6))


def grad_norm64(g):
    with np.errstate(all="ignore"):
        return math.sqrt(sum(float(np.sum(np.square(np.asarray(x, dtype=np.float64)))) for x in g))


def lerp64(a, b, w):
    """torch.lerp: a + w (b - a), which torch evaluates from the nearer end (b - (b - a)(1 - w) for w >= 0.5).  The two
    agree in exact arithmetic; following torch keeps the float64 comparison with it at 1e-12 where a and b cancel."""
    return a + w * (b - a) if w < 0.5 else b - (b - a) * (1.0 - w)


def clip_adam_step64(p, g, m, v, *, step, lr, betas, eps, weight_decay, max_norm, norm=None):
    """One clip + Adam step at the 1-based Adam step `step` over lists of arrays; m[i] is None for a clip-only tensor
    (in the norm, gradient scaled, nothing else: p'[i], m'[i], v'[i] are None).  `norm`: evaluate the element-wise
    update under this global norm (the kernel's own) instead of the float64 one; norm64 is returned either way."""
    b1, b2 = betas
    norm64 = grad_norm64(g)
    coef = clip_coef64(norm64 if norm is None else norm, max_norm)
    bc1 = 1.0 - b1 ** step
    bc2 = 1.0 - b2 ** step
    P, G, M, V = [], [], [], []
    with np.errstate(all="ignore"):
        for pi, gi, mi, vi in zip(p, g, m, v):
            gc = np.asarray(gi, dtype=np.float64) * coef
            G.append(gc)
            if mi is None:
                P.append(None); M.append(None); V.append(None)
                continue
            p64, m64, v64 = (np.asarray(x, dtype=np.float64) for x in (pi, mi, vi))
            # torch skips the term at weight_decay == 0.  That matters only for a parameter that is already not finite:
            # the kernel's fmaf(0, NaN, g) then makes both moments NaN, where torch keeps the second one
            ge = gc + weight_decay * p64 if weight_decay != 0 else gc
            m2 = lerp64(m64, ge, 1.0 - b1)
            v2 = b2 * v64 + (1.0 - b2) * ge * ge
            P.append(p64 - (lr / bc1) * m2 / (np.sqrt(v2) / math.sqrt(bc2) + eps))
            M.append(m2); V.append(v2)
    return P, G, M, V, norm64


# ---------------------------------------------------------------------------------------------------------------------
# the hyper-parameter rows and inputs that the CPU sensitivity test and the GPU test share
# ---------------------------------------------------------------------------------------------------------------------
_DEFAULTS = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-6, max_norm=1.0)         # train.py:96,141
HYPER = {
    "defaults": dict(_DEFAULTS),
    "moved": dict(lr=1e-2, betas=(0.5, 0.9), eps=1e-3, weight_decay=0.1, max_norm=0.5),
    "zero_betas": dict(_DEFAULTS, betas=(0.0, 0.0)),
    "lr0": dict(_DEFAULTS, lr=0.0),
    "nowd_noclip": dict(_DEFAULTS, weight_decay=0.0, max_norm=None),
    "nowd_max0": dict(_DEFAULTS, weight_decay=0.0, max_norm=0.0),
}
STEPS = (1, 2, 1000)
# total gradient norm as a multiple of max_norm (of 1 where there is no max_norm): well inside either side of the clip
SIDES = {"unclipped": 0.25, "clipped": 4.0}
HYPER_SIZES = (1023, 16385, 5)            # optimised tensors of the hyper-parameter cases ...
HYPER_CLIP_ONLY = (255,)                  # ... and a clip-only one


def make_inputs(sizes, clip_only_sizes, *, seed, step, norm, max_norm):
    """fp32 inputs of one step: parameters at the model's init scale 0.02, gradients of total norm `norm` (clip-only
    tensors, which come last, included), and for step > 1 moments at the scale of the gradient that Adam will see
    (first moment 0.5 x that scale, second moment between 0.5 and 1.5 x its square, so never near 0, like a running
    mean of squares); zeros at step 1.  Returns the `before` dict of compare_step."""
    rng = np.random.RandomState(seed)
    sizes, clip_only_sizes = list(sizes), list(clip_only_sizes)
    g = [rng.standard_normal(n) for n in sizes + clip_only_sizes]
    total = math.sqrt(sum(float(np.sum(x * x)) for x in g))
    g = [(x * (norm / total)).astype(np.float32) for x in g]
    seen = (min(norm, max_norm) if max_norm else norm) / math.sqrt(sum(sizes + clip_only_sizes))
    p, m, v = [], [], []
    for n in sizes:
        p.append((0.02 * rng.standard_normal(n)).astype(np.float32))
        if step == 1:
            m.append(np.zeros(n, np.float32)); v.append(np.zeros(n, np.float32))
        else:
            m.append((0.5 * seen * rng.standard_normal(n)).astype(np.float32))
            v.append((seen * seen * (0.5 + rng.random_sample(n))).astype(np.float32))
    none = [None] * len(clip_only_sizes)
    return dict(p=p + none, g=g, m=m + none, v=v + none)


# ---------------------------------------------------------------------------------------------------------------------
# comparison of a stored fp32 step with the model
# ---------------------------------------------------------------------------------------------------------------------
def _same_nonfinite(a, b, what):
    """NaN where the model has NaN, the model's infinity where it has one; returns the mask of the model's finite elements."""
    if a.shape != b.shape:
        raise AssertionError(f"{what}: shape {a.shape} != {b.shape}")
    fin = np.isfinite(b)
    if not np.array_equal(np.isnan(a), np.isnan(b)):
        raise AssertionError(f"{what}: NaN at other elements than the model's")
    inf = np.isinf(b)
    if not np.array_equal(np.isinf(a), inf) or not np.array_equal(a[inf], b[inf]):
        raise AssertionError(f"{what}: infinities differ from the model's")
    return fin


def elem_err_nf(a, b, what):
    """helpers.elem_err (|a - b| / max(|b|, rms(b))) over the model's finite elements; the others must coincide."""
    from helpers import elem_err
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    fin = _same_nonfinite(a, b, what)
    return elem_err(a[fin], b[fin])


def compare_step(before, after, norm_kernel, *, step, lr, betas, eps, weight_decay, max_norm):
    """Hold one stored step to clip_adam_step64.

    before / after: dicts of lists "p", "g", "m", "v" of float32 arrays (p, m, v None for a clip-only tensor);
    norm_kernel: the norm the step reported.  Raises AssertionError at the first quantity out of bounds, else returns
    the worst value of each: norm (relative), g, m, v (elem_err), dp (elem_err of the update, without the rounding
    allowance), dp_bound (largest |dp - dp64| as a fraction of its bound).

      norm   |norm_kernel - norm64| <= 1e-5 norm64 (both NaN, or both the same infinity, when the model's is not finite)
      g      bit-equal to before where max_norm is None or <= 0 or norm64 <= max_norm / 2;
             elem_err <= 2e-6 of the model under norm_kernel where norm64 >= 2 max_norm or norm64 is not finite;
             a norm in between is refused (the case would be ambiguous)
      m, v   elem_err <= 2e-6
      dp     per element |dp - dp64| <= 2e-6 max(|dp64|, rms(dp64)) + ulp32(max(|p_before|, |p_after|)) / 2,
             the last term being the one rounding of the stored parameter"""
    hp = dict(step=step, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, max_norm=max_norm)
    P, G, M, V, norm64 = clip_adam_step64(before["p"], before["g"], before["m"], before["v"], norm=float(norm_kernel), **hp)
    worst = dict(norm=0.0, g=0.0, m=0.0, v=0.0, dp=0.0, dp_bound=0.0)
    nk = float(norm_kernel)
    if math.isfinite(norm64):
        worst["norm"] = abs(nk - norm64) / norm64 if norm64 > 0 else (0.0 if nk == 0.0 else float("inf"))
        assert worst["norm"] <= NORM_TOL, ("norm", nk, norm64)
    else:
        assert (nk != nk) if norm64 != norm64 else nk == norm64, ("norm", nk, norm64)
    unclipped = max_norm is None or max_norm <= 0 or norm64 <= max_norm / 2
    if not unclipped and math.isfinite(norm64) and norm64 < 2 * max_norm:
        raise ValueError(f"norm {norm64} within a factor 2 of max_norm {max_norm}: move the case off the threshold")
    for i, (gb, ga, g64) in enumerate(zip(before["g"], after["g"], G)):
        if unclipped:
            assert np.array_equal(np.asarray(ga).view(np.uint32), np.asarray(gb).view(np.uint32)), ("g not bit-equal", i)
        else:
            e = elem_err_nf(ga, g64, f"g[{i}]")
            worst["g"] = max(worst["g"], e)
            assert e <= TOL, ("g", i, e)
    for i in range(len(P)):
        if P[i] is None:
            assert after["p"][i] is None and after["m"][i] is None and after["v"][i] is None
            continue
        for k, ref in (("m", M[i]), ("v", V[i])):
            e = elem_err_nf(after[k][i], ref, f"{k}[{i}]")
            worst[k] = max(worst[k], e)
            assert e <= TOL, (k, i, e)
        pb, pa = np.asarray(before["p"][i], dtype=np.float32), np.asarray(after["p"][i], dtype=np.float32)
        p_ref = np.asarray(P[i], dtype=np.float64)
        fin = _same_nonfinite(pa.astype(np.float64), p_ref, f"p[{i}]")
        if not fin.any():
            continue
        pb, pa, p_ref = pb[fin], pa[fin], p_ref[fin]
        dp = pa.astype(np.float64) - pb.astype(np.float64)
        dp64 = p_ref - pb.astype(np.float64)
        scale = np.maximum(np.abs(dp64), float(np.sqrt(np.mean(dp64 * dp64))))
        half_ulp = 0.5 * np.spacing(np.maximum(np.abs(pb), np.abs(pa))).astype(np.float64)
        diff = np.abs(dp - dp64)
        bound = TOL * scale + half_ulp
        worst["dp_bound"] = max(worst["dp_bound"], float((diff / bound).max()))
        worst["dp"] = max(worst["dp"], float((np.maximum(diff - half_ulp, 0.0) / np.maximum(scale, 1e-300)).max()))
        assert (diff <= bound).all(), ("dp", i, float((diff / bound).max()))
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# the training meter's record
# ---------------------------------------------------------------------------------------------------------------------
def _fmin(a, b):
    """C fmin / fminf: the other operand when one is NaN."""
    if a != a:
        return b
    if b != b:
        return a
    return min(a, b)


def meter64(state, capacity, total, vertex_loss, existence_loss, edge_loss, pred0, tgt0, count0=None):
    """The record after one update.  state: 8 + capacity values (steps, best total loss, best RMSE, last total / vertex /
    existence / edge loss, last RMSE, then the ring: step t at 8 + t % capacity).  Losses are numbers (None: the key is
    missing, the record holds 0).  pred0 [Vp, 3], tgt0 [Vt, 3]: sample 0; RMSE = sqrt(mean((pred - target)^2)) over the
    first clamp(count0, 0, min(Vp, Vt)) vertices x 3 coordinates (count0 None: all of them), 0 when there is none.
    The minima start at the first step and follow fminf: a NaN never replaces a number, a number replaces a NaN."""
    s = np.array(state, dtype=np.float64)
    assert s.shape == (8 + capacity,)
    max_v = min(len(pred0), len(tgt0))
    c = max_v if count0 is None else min(max(int(count0), 0), max_v)
    if c > 0:
        d = np.asarray(pred0[:c], dtype=np.float64)[:, :3] - np.asarray(tgt0[:c], dtype=np.float64)[:, :3]
        rmse = math.sqrt(float(np.sum(d * d)) / (3 * c))
    else:
        rmse = 0.0
    step = int(s[0])
    t = float(total)
    s[1] = t if step == 0 else _fmin(s[1], t)
    s[2] = rmse if step == 0 else _fmin(s[2], rmse)
    s[3] = t
    s[4], s[5], s[6] = (0.0 if x is None else float(x) for x in (vertex_loss, existence_loss, edge_loss))
    s[7] = rmse
    if capacity > 0:
        s[8 + step % capacity] = t
    s[0] = step + 1
    return s
