"""No kernel runs here.  (1) wf3d.optim.lr_factor, the schedules' specification, against torch's own schedulers in
float64; (2) tests/optim_sched_model.py's EMA model against torch, and its comparison routine against near misses of the
step it describes; (3) what wf3d.optim.ClipAdam accepts, refuses, saves and loads for `lr_schedule`, `ema_decay` and
`schedule_step`, on CPU tensors."""
import warnings

import numpy as np
import pytest
import torch

import helpers as H  # noqa: F401  (puts the package on sys.path)
import optim_groups_model as GM
import optim_model as OM
import optim_sched_model as SM

TG = list(GM.TENSOR_GROUP) + [None]


# ---------------------------------------------------------------------------------------------------------------------
# 1. lr_factor against torch.optim.lr_scheduler
# ---------------------------------------------------------------------------------------------------------------------
W, T, LR = 5, 20, 3e-3
CASES = {
    "warmup_cosine": (dict(warmup_steps=W, warmup_start=0.01, decay="cosine", decay_steps=T, min_factor=0.01), W + T),
    "cosine": (dict(decay="cosine", decay_steps=T, min_factor=0.1), T),
    "warmup_linear": (dict(warmup_steps=W, warmup_start=0.25, decay="linear", decay_steps=T, min_factor=0.05), W + T),
    "warmup_multistep": (dict(warmup_steps=W, warmup_start=0.5, decay="multistep", gamma=0.5, milestones=(3, 3, 7)), W + 10),
    "exponential": (dict(decay="exponential", gamma=0.9), 30),
    "warmup": (dict(warmup_steps=W, warmup_start=0.1), W + 3),
}


def _torch_rates(schedule, last):
    """The rate torch applies at t = 0..last: group["lr"] after t scheduler steps, Python floats (float64)."""
    from torch.optim import lr_scheduler as LS
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1, dtype=torch.float64))], lr=LR)
    s = dict(dict(warmup_steps=0, warmup_start=0.0, decay="constant", min_factor=0.0), **schedule)
    parts = []
    if s["warmup_steps"]:
        parts.append(LS.LinearLR(opt, start_factor=s["warmup_start"], end_factor=1.0, total_iters=s["warmup_steps"]))
    if s["decay"] == "cosine":
        parts.append(LS.CosineAnnealingLR(opt, T_max=s["decay_steps"], eta_min=LR * s["min_factor"]))
    elif s["decay"] == "linear":
        parts.append(LS.LinearLR(opt, start_factor=1.0, end_factor=s["min_factor"], total_iters=s["decay_steps"]))
    elif s["decay"] == "multistep":
        parts.append(LS.MultiStepLR(opt, milestones=list(s["milestones"]), gamma=s["gamma"]))
    elif s["decay"] == "exponential":
        parts.append(LS.ExponentialLR(opt, gamma=s["gamma"]))
    sched = parts[0] if len(parts) == 1 else LS.SequentialLR(opt, parts, milestones=[s["warmup_steps"]])
    rates = []
    for _ in range(last + 1):
        rates.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
    return rates


@pytest.mark.parametrize("case", sorted(CASES))
def test_lr_factor_is_torchs_schedulers_composed_by_sequential_lr(case):
    from wf3d.optim import lr_factor
    schedule, last = CASES[case]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rates = _torch_rates(schedule, last)
    worst = 0.0
    for t, want in enumerate(rates):
        got = LR * lr_factor(schedule, t)
        assert isinstance(want, float)
        worst = max(worst, abs(got - want) / abs(want))
    print(f"[lr_factor] {case}: {len(rates)} steps, largest relative difference from torch {worst:.1e}")
    assert worst <= 1e-12
    assert len({round(r, 15) for r in rates}) > 2               # the case does change the rate


def test_cosine_and_linear_stay_at_min_factor_past_the_end():
    from wf3d.optim import lr_factor
    for kind in ("cosine", "linear"):
        s = dict(warmup_steps=3, warmup_start=0.5, decay=kind, decay_steps=10, min_factor=0.125)
        assert lr_factor(s, 12) > 0.125
        for t in (13, 14, 23, 1000, 2 ** 24 + 1, 2 ** 40):
            assert lr_factor(s, t) == pytest.approx(0.125, rel=1e-15), (kind, t)
    assert lr_factor(dict(decay="exponential", gamma=0.5, min_factor=0.125), 2) == 0.25
    assert [lr_factor(dict(decay="exponential", gamma=0.5, min_factor=0.125), t) for t in (3, 4, 10 ** 6)] == [0.125] * 3


def test_a_milestone_counts_from_the_update_it_names():
    from wf3d.optim import lr_factor
    s = dict(warmup_steps=2, warmup_start=0.5, decay="multistep", gamma=0.5, milestones=(0, 3, 3, 5))
    # u = max(t - 2, 0): milestone 0 holds from the start (u is 0 all through the warm-up), the repeated 3 counts twice,
    # and each milestone counts from u == m on
    assert [lr_factor(s, t) for t in range(9)] == [0.25, 0.375, 0.5, 0.5, 0.5, 0.125, 0.125, 0.0625, 0.0625]


def test_an_empty_schedule_is_exactly_one():
    from wf3d.optim import lr_factor
    for s in (None, {}):
        for t in (0, 1, 7, 2 ** 24 + 1):
            f = lr_factor(s, t)
            assert isinstance(f, float) and f == 1.0
    assert SM.applied_lr(1e-3, None, 5) == float(np.float32(1e-3))


# ---------------------------------------------------------------------------------------------------------------------
# 2. the EMA model and the comparison routine
# ---------------------------------------------------------------------------------------------------------------------
def test_ema_step64_is_torchs_ema_at_constant_decay():
    from torch.optim.swa_utils import get_ema_avg_fn
    rng = np.random.RandomState(0)
    e, p = rng.standard_normal(1000), rng.standard_normal(1000)
    for d in (0.999, 0.9, 0.5, 0.1):
        want = get_ema_avg_fn(d)(torch.from_numpy(e), torch.from_numpy(p), 7).numpy()
        lerp = torch.lerp(torch.from_numpy(e), torch.from_numpy(p), 1.0 - d).numpy()
        got = SM.ema_step64(e, p, SM.ema_decay64(d, False, 123))
        assert got.dtype == np.float64
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
        assert np.abs(got - lerp).max() <= 1e-12 * np.abs(lerp).max()


def test_ema_warmup_is_the_written_out_formula():
    for n, want in ((0, 0.1), (1, 2 / 11), (2, 0.25), (90, 0.91), (8990, 0.999)):
        assert SM.ema_decay64(0.9995, True, n) == pytest.approx(want, rel=1e-15)
    assert SM.ema_decay64(0.999, True, 8990) == 0.999 == SM.ema_decay64(0.999, True, 10 ** 6)      # the cap
    assert SM.ema_decay64(0.999, True, 999) == (1.0 + 999) / (10.0 + 999)
    assert SM.ema_decay64(0.999, False, 0) == 0.999
    e, p = np.array([1.0, -2.0]), np.array([3.0, 2.0])
    assert np.array_equal(SM.ema_step64(e, p, 0.25), np.array([2.5, 1.0]))


DECAY = [0.999, 0.99]
SCHEDULES = [dict(warmup_steps=4, warmup_start=0.25), dict(decay="multistep", gamma=0.5, milestones=(1,))]


def _cases():
    for steps in GM.GROUP_STEPS:
        for side in sorted(OM.SIDES):
            yield steps, side


def _before(steps, side, t=1):
    seed = 100 * GM.GROUP_STEPS.index(steps) + sorted(OM.SIDES).index(side)
    b = GM.make_group_inputs(OM.HYPER_SIZES, OM.HYPER_CLIP_ONLY, GM.TENSOR_GROUP, steps, seed=seed, norm=OM.SIDES[side] * GM.MAX_NORM)
    return SM.add_averages(b, TG, DECAY, seed + 1, t=t)


def _rejected(mutation, steps, side):
    groups = GM.two_groups(steps)
    before = _before(steps, side)
    kw = dict(group=TG, groups=groups, max_norm=GM.MAX_NORM, schedules=SCHEDULES, ema_decay=DECAY, ema_warmup=True)
    hooks, skipped = {}, False
    if mutation == "d_and_one_minus_d_exchanged":
        hooks = dict(d_of=lambda d, n, k: 1.0 - d)
    elif mutation == "average_of_the_parameter_before_the_update":
        hooks = dict(ema_of="before")
    elif mutation == "warmup_at_n_plus_1":
        hooks = dict(d_of=lambda d, n, k: SM.ema_decay64(DECAY[k], True, n + 1))
    elif mutation == "factor_at_t_plus_1":
        hooks = dict(at=before["t"] + 1)
    after, norm = SM.store32(before, TG, groups, GM.MAX_NORM, t=before["t"], schedules=SCHEDULES, ema_decay=DECAY, ema_warmup=True,
                             **hooks)
    if mutation == "factor_at_t_plus_1":
        after["lr"] = None                                      # the update alone must give it away
    elif mutation == "average_moved_in_a_skipped_step":
        after, skipped = dict(before, e=after["e"]), True
    elif mutation == "count_moved_in_a_skipped_step":
        after, skipped = dict(before, t=before["t"] + 1), True
    elif mutation == "skipped":
        after, skipped = dict(before), True
    try:
        SM.compare_sched_step(before, after, norm, skipped=skipped, **kw)
    except AssertionError:
        return True
    return False


def test_comparison_accepts_the_model_stored_in_fp32():
    for case in _cases():
        assert not _rejected(None, *case), case
        assert not _rejected("skipped", *case), case
    assert OM.clip_adam_step64 is GM._single_step64


# the warm-up's d moves with n wherever it is below its cap: (1 + n) / (10 + n) is 0.99108 at n = 999, below group 0's 0.999
# (group 1 sits at its cap 0.99 there), so every case has a group that shows n + 1
MUTATIONS = ["d_and_one_minus_d_exchanged", "average_of_the_parameter_before_the_update", "warmup_at_n_plus_1",
             "average_moved_in_a_skipped_step", "count_moved_in_a_skipped_step", "factor_at_t_plus_1"]


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_comparison_rejects_a_near_miss(mutation):
    missed = [c for c in _cases() if not _rejected(mutation, *c)]
    assert not missed, (mutation, missed)


# ---------------------------------------------------------------------------------------------------------------------
# 3. ClipAdam's constructor, add_param_group, state_dict and load_state_dict, on CPU tensors
# ---------------------------------------------------------------------------------------------------------------------
def _params(n):
    return [torch.nn.Parameter(torch.zeros(3)) for _ in range(n)]


COSINE = dict(warmup_steps=500, warmup_start=0.01, decay="cosine", decay_steps=20000, min_factor=0.01)


def test_groups_inherit_the_new_defaults_and_override_them():
    from wf3d.optim import ClipAdam
    a, b, c = _params(3)
    opt = ClipAdam([dict(params=[a]), dict(params=[b], lr_schedule=None, ema_decay=0), dict(params=[c], lr_schedule=dict(warmup_steps=3))],
                   lr=1e-3, lr_schedule=COSINE, ema_decay=0.999, ema_warmup=True)
    g0, g1, g2 = opt.param_groups
    assert g0["lr_schedule"] == dict(COSINE, gamma=1.0, milestones=()) and g0["ema_decay"] == 0.999
    assert g1["lr_schedule"] is None and g1["ema_decay"] == 0
    assert g2["lr_schedule"]["warmup_steps"] == 3 and g2["lr_schedule"]["decay"] == "constant" and g2["ema_decay"] == 0.999
    assert all(g["lr"] == 1e-3 for g in opt.param_groups)       # the base rate, untouched by the schedule
    assert opt.ema_warmup is True and opt.schedule_step == 0 and opt.last_lr is None
    plain = ClipAdam([a])
    assert plain.param_groups[0]["lr_schedule"] is None and plain.param_groups[0]["ema_decay"] is None
    cap = ClipAdam([a], capturable=True, lr_schedule=COSINE)
    assert cap.schedule_step is None                            # created on the device by the first step
    cap.set_schedule_step(7)
    assert cap.state_dict()["schedule_step"] == 7


BAD = [dict(warmup=3), dict(decay="cosine_restarts", decay_steps=5), dict(warmup_steps=-1), dict(decay="cosine"),
       dict(decay="cosine", decay_steps=0), dict(decay="linear", decay_steps=0), dict(warmup_steps=2, warmup_start=1.5),
       dict(warmup_steps=2, warmup_start=-0.1), dict(decay="linear", decay_steps=4, min_factor=1.01),
       dict(decay="exponential"), dict(decay="exponential", gamma=0.0), dict(decay="exponential", gamma=1.5),
       dict(decay="multistep", gamma=0.5, milestones=tuple(range(9))), dict(decay="multistep", gamma=0.5, milestones=(3, 2)),
       dict(decay="multistep", milestones=(3,)), "cosine"]


@pytest.mark.parametrize("bad", BAD, ids=[str(i) for i in range(len(BAD))])
def test_a_bad_schedule_is_refused_everywhere(bad):
    from wf3d.optim import ClipAdam
    a, b = _params(2)
    with pytest.raises(ValueError, match="lr_schedule"):
        ClipAdam([a], lr_schedule=bad)
    with pytest.raises(ValueError, match="lr_schedule"):
        ClipAdam([dict(params=[a]), dict(params=[b], lr_schedule=bad)])
    opt = ClipAdam([a])
    with pytest.raises(ValueError, match="lr_schedule"):
        opt.add_param_group(dict(params=[b], lr_schedule=bad))
    assert len(opt.param_groups) == 1


def test_eight_milestones_with_repeats_are_accepted():
    from wf3d.optim import ClipAdam
    opt = ClipAdam(_params(1), lr_schedule=dict(decay="multistep", gamma=0.5, milestones=[1, 1, 2, 3, 5, 8, 8, 13]))
    assert opt.param_groups[0]["lr_schedule"]["milestones"] == (1, 1, 2, 3, 5, 8, 8, 13)


def test_a_schedule_beside_a_tensor_lr_and_bad_decays_are_refused():
    from wf3d.optim import ClipAdam
    a, b = _params(2)
    lr = torch.tensor(1e-3)
    with pytest.raises(ValueError, match="not both"):
        ClipAdam([a], lr=lr, capturable=True, lr_schedule=COSINE)
    opt = ClipAdam([a], capturable=True, lr_schedule=COSINE)
    with pytest.raises(ValueError, match="not both"):
        opt.add_param_group(dict(params=[b], lr=lr))
    opt.add_param_group(dict(params=[b], lr=lr, lr_schedule=None))           # a tensor lr beside a scheduled group is fine
    assert len(opt.param_groups) == 2
    for bad in (1.0, -0.1, "0.9", True):
        with pytest.raises(ValueError, match="ema_decay"):
            ClipAdam(_params(1), ema_decay=bad)
    with pytest.raises(TypeError, match="ema_warmup"):
        ClipAdam(_params(1), ema_decay=0.9, ema_warmup=1)
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match="schedule_step"):
            ClipAdam(_params(1)).set_schedule_step(bad)


def test_state_dicts_travel_between_clip_adam_and_torch_adam():
    from wf3d.optim import ClipAdam
    a, b = _params(2)
    opt = ClipAdam([dict(params=[a], lr=1e-4, lr_schedule=COSINE), dict(params=[b], ema_decay=None)], lr=1e-3, ema_decay=0.99)
    for p in (a, b):
        opt.state[p] = {"step": torch.tensor(3.0), "exp_avg": torch.ones(3), "exp_avg_sq": torch.ones(3)}
    opt.state[a]["ema"] = torch.full((3,), 0.5)
    opt.set_schedule_step(41)
    sd = opt.state_dict()
    assert sd["schedule_step"] == 41 and sd["param_groups"][0]["lr"] == 1e-4 and torch.equal(sd["state"][0]["ema"], torch.full((3,), 0.5))
    # ClipAdam -> ClipAdam: the count, the schedules, the decays and the averages
    c, d = _params(2)
    twin = ClipAdam([dict(params=[c]), dict(params=[d])])
    twin.load_state_dict(sd)
    assert twin.schedule_step == 41 and twin.param_groups[0]["lr_schedule"] == opt.param_groups[0]["lr_schedule"]
    assert [g["ema_decay"] for g in twin.param_groups] == [0.99, None] and torch.equal(twin.state[c]["ema"], torch.full((3,), 0.5))
    assert "ema" not in twin.state[d]
    # ClipAdam -> torch.optim.Adam
    ref = torch.optim.Adam([dict(params=[c]), dict(params=[d])])
    ref.load_state_dict(sd)
    assert ref.param_groups[0]["lr"] == 1e-4 and float(ref.state[c]["step"]) == 3.0
    # torch.optim.Adam -> ClipAdam: the new keys take this optimizer's defaults, the count is 0
    fresh = torch.optim.Adam([dict(params=[c], lr=0.5), dict(params=[d])])
    back = ClipAdam([dict(params=[c]), dict(params=[d])], lr_schedule=dict(warmup_steps=2), ema_decay=0.9)
    back.set_schedule_step(9)
    back.load_state_dict(fresh.state_dict())
    assert back.schedule_step == 0 and back.param_groups[0]["lr"] == 0.5
    assert all(g["lr_schedule"]["warmup_steps"] == 2 and g["ema_decay"] == 0.9 for g in back.param_groups)
    bad = opt.state_dict()
    bad["param_groups"][0]["lr_schedule"] = dict(decay="nope")
    with pytest.raises(ValueError, match="lr_schedule"):
        twin.load_state_dict(bad)


def test_the_new_entry_points_check_their_arguments():
    """Argument checks only: nothing is launched."""
    import ctypes
    from wf3d import _lib
    lib = _lib.load()
    vp, E = ctypes.c_void_p, _lib.DEFINES
    assert E["WF3D_ADAM_SKIP_NONFINITE"] == 1 and E["WF3D_ADAM_EMA_WARMUP"] == 2
    from wf3d.optim import DECAYS
    assert [E[f"WF3D_LR_{k.upper()}"] for k in DECAYS] == [0, 1, 2, 3, 4]
    tab = (vp * 2)(0x1000, 0x1000)                              # never dereferenced: the checks come first
    d2, i2, l2 = (ctypes.c_double * 2)(0.5, 0.5), (ctypes.c_int * 2)(1, 1), (ctypes.c_long * 2)(4, 4)

    def step(ema=None, ema_decay=d2, flags=0, steps=None, sched=None):
        return lib.wf3d_clip_adam_step_ema(tab, tab, tab, tab, ema, l2, (ctypes.c_int * 2)(0, 1), steps, 2, d2, None, d2, d2, d2, d2,
                                           i2, ema_decay, i2, 2, 1.0, flags, None, sched, None, 0, None, None)
    assert step() == E["WF3D_ERR_WS"]                           # past every argument check, stopped before the first launch
    assert step(flags=4) == E["WF3D_ERR_ARG"] and b"unknown flags" in lib.wf3d_last_error()
    assert step(flags=2) == E["WF3D_ERR_WS"]
    assert step(sched=0x1000) == E["WF3D_ERR_ARG"] and b"schedule_step needs device step counters" in lib.wf3d_last_error()
    assert step(ema=tab, ema_decay=None) == E["WF3D_ERR_ARG"] and b"ema_decay" in lib.wf3d_last_error()
    assert step(ema=tab, ema_decay=(ctypes.c_double * 2)(0.5, 1.0)) == E["WF3D_ERR_ARG"] and b"outside [0, 1)" in lib.wf3d_last_error()
    assert step(ema=tab, ema_decay=(ctypes.c_double * 2)(0.5, 0.0)) == E["WF3D_ERR_ARG"] and b"tensor 1 has an average" in lib.wf3d_last_error()
    assert step(ema=tab) == E["WF3D_ERR_WS"]

    def sched(**kw):
        row = dict(warmup_steps=l2, warmup_start=d2, decay=i2, decay_steps=l2, min_factor=d2, gamma=d2,
                   milestones=(ctypes.c_long * 16)(*[0] * 16), nmilestones=(ctypes.c_int * 2)(0, 0), ngroups=2)
        row.update(kw)
        return lib.wf3d_lr_schedule(d2, row["warmup_steps"], row["warmup_start"], row["decay"], row["decay_steps"], row["min_factor"],
                                    row["gamma"], row["milestones"], row["nmilestones"], i2, row["ngroups"], 0x1000, None, None)
    assert sched() == E["WF3D_ERR_ARG"] and b"null table" in lib.wf3d_last_error()          # last_lr
    assert sched(ngroups=17) == E["WF3D_ERR_UNSUPPORTED"]
    assert lib.wf3d_ema_swap(tab, None, l2, 2, None) == E["WF3D_ERR_ARG"]
    assert lib.wf3d_ema_swap(tab, tab, l2, 2, None) == E["WF3D_ERR_ARG"] and b"lacks a side" in lib.wf3d_last_error()
