"""A float64 model of what the step tail does beside clip + Adam (csrc/optim.hip, wf3d.optim.ClipAdam): the averaged
weights and the learning-rate schedule's place in a step.  It stands on tests/optim_groups_model.py (the grouped step)
and on wf3d.optim.lr_factor, the schedule's specification.

  ema_decay64(decay, warmup, n)             the decay d of one update: decay, or min(decay, (1 + n) / (10 + n))
  ema_step64(ema, p_new, d)                 ema + (1 - d) (p_new - ema), float64
  applied_lr(lr, schedule, t)               float32(lr * lr_factor(schedule, t)), as a Python float
  compare_sched_step(before, after, ...)    a stored fp32 step against all of it, and its bounds

tests/test_optim_sched_model.py pins these to torch (its schedulers, swa_utils' EMA) and shows that compare_sched_step
rejects near misses; tests/test_optim_sched_gpu.py holds the kernels to it."""
import numpy as np

import optim_groups_model as GM


def ema_decay64(decay, warmup, n):
    """n: the tensor's Adam step BEFORE the update (0 for its first)."""
    return min(decay, (1.0 + n) / (10.0 + n)) if warmup else float(decay)


def ema_step64(ema, p_new, d):
    ema, p_new = np.asarray(ema, dtype=np.float64), np.asarray(p_new, dtype=np.float64)
    return ema + (1.0 - d) * (p_new - ema)


def ema_bound(ema_new, p_new, ema, d):
    """2^-23 (|ema'| + 2 (1 - d) |p' - ema|): the difference p' - ema and the fp32 value of 1 - d each carry one rounding
    of 2^-24 relative into the product term, the fma rounds the result once more by 2^-24 of |ema'|; a factor 2 of
    margin on their sum."""
    return 2.0 ** -23 * (np.abs(ema_new) + 2.0 * (1.0 - d) * np.abs(np.asarray(p_new, np.float64) - np.asarray(ema, np.float64)))


def applied_lr(lr, schedule, t):
    from wf3d.optim import lr_factor
    return float(np.float32(lr * lr_factor(schedule, t)))


def neighbours32(x):
    """x as fp32 and the fp32 values on either side of it."""
    x = np.float32(x)
    return {float(x), float(np.nextafter(x, np.float32(np.inf))), float(np.nextafter(x, np.float32(-np.inf)))}


def _bits_equal(a, b):
    return (a is None and b is None) or (a is not None and b is not None and
                                         np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32)))


def compare_sched_step(before, after, norm_kernel, *, group, groups, max_norm, schedules=None, ema_decay=None,
                       ema_warmup=False, skipped=False, lr_ulps=0):
    """Hold one stored step to the model.

    before / after: the dicts of optim_model.compare_step ("p", "g", "m", "v": lists of float32 arrays, None for what a
    clip-only tensor lacks) with "e" (the averages; None for a tensor without one) and "t" (the schedules' count of
    applied updates); after["lr"] (optional): the applied rates the step reported, one per group.
    group[i], groups: as optim_groups_model.compare_groups_step takes them; a row's "lr" is the BASE rate and its "step"
    the 1-based Adam step of this update.  schedules[k]: group k's schedule (None: none).  ema_decay[k]: group k's decay
    (None or 0: no average); ema_warmup as ClipAdam's.  lr_ulps: how many fp32 neighbours of float32(lr * factor) a
    reported rate may be away (0 on the host, 1 for the device's cos / pow).

    skipped: nothing may have moved, the averages and the count included.  Otherwise
      rate   after["lr"][k] is float32(lr_k * lr_factor(schedule_k, before["t"])) (within lr_ulps), and the step is
             held to compare_groups_step's bounds AT that rate: the factor belongs to the count before the step
      t      after["t"] == before["t"] + 1 where a parameter was updated and some group has a schedule (the count exists
             for the schedules), else before["t"]
      e      |e' - ema_step64(e, p', d)| <= ema_bound, from the STORED new parameter p' = after["p"], with
             d = ema_decay64(decay_k, ema_warmup, step_k - 1); a tensor without average has none before or after
    Returns compare_groups_step's worst values plus "e" (the largest fraction of its bound)."""
    n = len(before["g"])
    schedules = schedules or [None] * len(groups)
    ema_decay = ema_decay or [None] * len(groups)
    if skipped:
        for r in "pgmve":
            for i in range(n):
                assert _bits_equal(before[r][i], after[r][i]), (f"{r}[{i}] moved in a skipped step")
        assert after["t"] == before["t"], ("the schedule count moved in a skipped step", before["t"], after["t"])
        return {}
    rows = []
    for k, hp in enumerate(groups):
        want = applied_lr(hp["lr"], schedules[k], before["t"])
        got = want
        if after.get("lr") is not None and schedules[k] is not None:
            got = float(after["lr"][k])
            near = neighbours32(want) if lr_ulps else {want}
            assert got in near, ("applied rate", k, got, want)
        rows.append(dict(hp, lr=got))
    core = lambda d: {r: d[r] for r in "pgmv"}      # noqa: E731
    worst = GM.compare_groups_step(core(before), core(after), norm_kernel, group=group, groups=rows, max_norm=max_norm)
    counted = any(g is not None for g in group) and any(s is not None for s in schedules)
    assert after["t"] == before["t"] + (1 if counted else 0), ("schedule count", before["t"], after["t"])
    worst["e"] = 0.0
    for i in range(n):
        k = group[i]
        if k is None or not ema_decay[k]:
            assert before["e"][i] is None and after["e"][i] is None, ("a tensor without average has one", i)
            continue
        d = ema_decay64(ema_decay[k], ema_warmup, groups[k]["step"] - 1)
        ref = ema_step64(before["e"][i], after["p"][i], d)
        bound = ema_bound(ref, after["p"][i], before["e"][i], d)
        diff = np.abs(np.asarray(after["e"][i], dtype=np.float64) - ref)
        frac = float((diff / np.maximum(bound, 1e-300)).max())
        worst["e"] = max(worst["e"], frac)
        assert (diff <= bound).all(), ("e", i, frac)
    return worst


def store32(before, group, groups, max_norm, *, t, schedules=None, ema_decay=None, ema_warmup=False, at=None,
            ema_of=None, d_of=None):
    """The model's step stored in fp32: the `after` dict of compare_sched_step, with the norm.  The keyword hooks build
    near misses: at (the count the factor is evaluated at, default t), ema_of("before" / "after": which parameter the
    average follows), d_of(d, n, k) -> the decay used in place of group k's d at Adam step n."""
    import optim_model as OM
    schedules = schedules or [None] * len(groups)
    ema_decay = ema_decay or [None] * len(groups)
    rows = [dict(hp, lr=applied_lr(hp["lr"], schedules[k], t if at is None else at)) for k, hp in enumerate(groups)]
    P, G, M, V, norm = GM.clip_adam_groups_step64(before["p"], before["g"], before["m"], before["v"], group, rows, max_norm)
    f32 = lambda xs: [None if x is None else np.asarray(x, dtype=np.float32) for x in xs]      # noqa: E731
    after = dict(p=f32(P), g=f32(G), m=f32(M), v=f32(V), e=[], t=before["t"] + 1, lr=[r["lr"] for r in rows])
    if OM.clip_coef64(norm, max_norm) == 1.0:
        after["g"] = [x.copy() for x in before["g"]]
    for i, k in enumerate(group):
        if k is None or not ema_decay[k]:
            after["e"].append(None)
            continue
        n = groups[k]["step"] - 1
        d = ema_decay64(ema_decay[k], ema_warmup, n)
        d = d_of(d, n, k) if d_of else d
        src = before["p"][i] if ema_of == "before" else after["p"][i]
        after["e"].append(ema_step64(before["e"][i], src, d).astype(np.float32))
    return after, np.float32(norm)


def add_averages(before, group, ema_decay, seed, t=0):
    """Averages about 0.01 away from the parameters (an average that lags them), for the tensors of averaged groups."""
    rng = np.random.RandomState(seed)
    e = []
    for p, k in zip(before["p"], group):
        has = k is not None and ema_decay[k]
        e.append((p + 0.01 * rng.standard_normal(p.shape)).astype(np.float32) if has else None)
    return dict(before, e=e, t=t)
