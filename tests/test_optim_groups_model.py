"""tests/optim_groups_model.py on the CPU: (1) clip_adam_groups_step64 against torch's own clip_grad_norm_ over all
tensors + Adam with two parameter groups (AdamW for a decoupled group) in float64; (2) compare_groups_step, at
optim_model's bounds and on the inputs of the GPU test, rejects a list of near misses of the grouped step;
(3) what wf3d.optim.ClipAdam accepts and refuses at construction and in add_param_group (no kernel runs here)."""
import numpy as np
import pytest
import torch

import helpers as H  # noqa: F401  (puts the package on sys.path)
import optim_groups_model as GM
import optim_model as OM


# ---------------------------------------------------------------------------------------------------------------------
# 1. the model against torch in float64
# ---------------------------------------------------------------------------------------------------------------------
def _torch_groups(tp, tensor_group, rows, which):
    return [dict(params=[q for q, k in zip(tp, tensor_group) if k == j], lr=rows[j]["lr"], betas=rows[j]["betas"],
                 eps=rows[j]["eps"], weight_decay=rows[j]["weight_decay"]) for j in which]


@pytest.mark.parametrize("form", ["two_l2_groups", "second_group_joins_after_two_steps", "second_group_decoupled",
                                  "first_group_decoupled"])
def test_model_matches_torch_clip_and_two_group_adam_in_float64(form):
    """Five steps on float64 CPU tensors: ONE clip_grad_norm_ over the tensors of both groups and a clip-only tensor,
    then torch.optim.Adam(foreach=False) over two groups whose lr, betas, eps and weight decay all differ; the tensors
    interleave (group 0, 1, 0).  `joins`: group 1 enters through add_param_group after two steps, so that it is at
    step 1 while group 0 is at step 3.  `decoupled`: that group steps through torch.optim.AdamW, the other through
    Adam.  Every p, g, m, v and the norm within 1e-12 (element-wise, of max(|x|, rms))."""
    rows = GM.TWO_GROUPS
    tensor_group = [0, 1, 0]
    rng = np.random.RandomState(11)
    sizes = [33, 200, 7]
    p = [0.02 * rng.standard_normal(n) for n in sizes] + [None]
    m = [np.zeros(n) for n in sizes] + [None]
    v = [np.zeros(n) for n in sizes] + [None]
    tp = [torch.nn.Parameter(torch.from_numpy(x.copy())) for x in p[:3]]
    lazy = torch.nn.Parameter(torch.zeros(50, dtype=torch.float64))
    decoupled = dict(second_group_decoupled=(False, True), first_group_decoupled=(True, False)).get(form, (False, False))
    joins = form == "second_group_joins_after_two_steps"
    if any(decoupled):
        cls = [torch.optim.AdamW if d else torch.optim.Adam for d in decoupled]
        opts = [cls[j](_torch_groups(tp, tensor_group, rows, [j]), foreach=False) for j in (0, 1)]
    else:
        opts = [torch.optim.Adam(_torch_groups(tp, tensor_group, rows, [0] if joins else [0, 1]), foreach=False)]
    taken = [0, 0]
    for it in range(1, 6):
        if joins and it == 3:
            opts[0].add_param_group(_torch_groups(tp, tensor_group, rows, [1])[0])
        live = [True, not joins or it >= 3]
        scale = 3.0 if it % 2 else 0.002                        # total norm about 50 and 0.03: both sides of max_norm
        g = [scale * rng.standard_normal(n) for n in sizes + [50]]
        for q, x in zip(tp + [lazy], g):
            q.grad = torch.from_numpy(x.copy())
        n_ref = float(torch.nn.utils.clip_grad_norm_(tp + [lazy], max_norm=GM.MAX_NORM))
        for o in opts:
            o.step()
        taken = [t + 1 if on else t for t, on in zip(taken, live)]
        groups = GM.two_groups(taken, decoupled)
        # a tensor whose group has not joined is, to the step, a clip-only one: in the norm, scaled, not updated
        tg = [k if live[k] else None for k in tensor_group] + [None]
        hide = [None if k is None else x for k, x in zip(tg, m)]
        P, G, M, V, n64 = GM.clip_adam_groups_step64(p, g, hide, v, tg, groups, GM.MAX_NORM)
        assert abs(n64 - n_ref) <= 1e-12 * n_ref
        for i, q in enumerate(tp + [lazy]):
            assert OM.elem_err_nf(G[i], q.grad.numpy(), "g") <= 1e-12
            if tg[i] is None:
                assert P[i] is None and M[i] is None and V[i] is None
                P[i], M[i], V[i] = p[i], m[i], v[i]
                continue
            st = [o for o in opts if q in o.state][0].state[q]
            assert int(st["step"]) == taken[tg[i]]
            assert OM.elem_err_nf(P[i], q.detach().numpy(), "p") <= 1e-12
            assert OM.elem_err_nf(M[i], st["exp_avg"].numpy(), "m") <= 1e-12
            assert OM.elem_err_nf(V[i], st["exp_avg_sq"].numpy(), "v") <= 1e-12
        p, m, v = P, M, V
    assert taken == ([5, 3] if joins else [5, 5])


def test_one_group_is_the_single_group_model():
    before = OM.make_inputs(OM.HYPER_SIZES, OM.HYPER_CLIP_ONLY, seed=3, step=2, norm=4.0, max_norm=1.0)
    hp = OM.HYPER["moved"]
    a = OM.clip_adam_step64(before["p"], before["g"], before["m"], before["v"], step=2, **hp)
    row = GM.group_hp(step=2, **{k: hp[k] for k in ("lr", "betas", "eps", "weight_decay")})
    b = GM.clip_adam_groups_step64(before["p"], before["g"], before["m"], before["v"], [0, 0, 0, None], [row], hp["max_norm"])
    assert a[4] == b[4]
    for x, y in zip(a[:4], b[:4]):
        for xi, yi in zip(x, y):
            assert (xi is None and yi is None) or np.array_equal(xi, yi)


# ---------------------------------------------------------------------------------------------------------------------
# 2. sensitivity: the GPU test's comparison must reject these
# ---------------------------------------------------------------------------------------------------------------------
TG = list(GM.TENSOR_GROUP) + [None]                             # the clip-only tensor comes last


def _mutant(mutation, before, groups):
    """The grouped step with one thing wrong (None: nothing)."""
    args = (before["p"], before["g"], before["m"], before["v"], TG)
    groups = [dict(r) for r in groups]
    if mutation == "per_group_norm":
        # each group (and the clip-only tensor) clipped by the norm of its own gradients
        out = [[None] * len(TG) for _ in range(4)]
        for k in (0, 1, None):
            idx = [i for i, t in enumerate(TG) if t == k]
            own = OM.grad_norm64([before["g"][i] for i in idx])
            res = GM.clip_adam_groups_step64(*args, groups, GM.MAX_NORM, norm=own)
            for r in range(4):
                for i in idx:
                    out[r][i] = res[r][i]
        return (*out, OM.grad_norm64(before["g"]))
    if mutation == "group0_lr_for_group1":
        groups[1]["lr"] = groups[0]["lr"]
    elif mutation == "l2_where_decoupled":
        groups = [dict(r, decoupled=False) for r in groups]
    elif mutation == "group0_step_for_group1":
        groups[1]["step"] = groups[0]["step"]
    else:
        assert mutation is None
    return GM.clip_adam_groups_step64(*args, groups, GM.MAX_NORM)


def _store32(x):
    with np.errstate(all="ignore"):
        return [None if a is None else np.asarray(a, dtype=np.float64).astype(np.float32) for a in x]


def _cases():
    for steps in GM.GROUP_STEPS:
        for decoupled in GM.DECAY_FORMS:
            for side in sorted(OM.SIDES):
                yield steps, decoupled, side


def _rejected(mutation, steps, decoupled, side):
    groups = GM.two_groups(steps, decoupled)
    seed = 100 * GM.GROUP_STEPS.index(steps) + 10 * GM.DECAY_FORMS.index(decoupled) + sorted(OM.SIDES).index(side)
    before = GM.make_group_inputs(OM.HYPER_SIZES, OM.HYPER_CLIP_ONLY, GM.TENSOR_GROUP, steps, seed=seed,
                                  norm=OM.SIDES[side] * GM.MAX_NORM)
    P, G, M, V, n64 = _mutant(mutation, before, groups)
    after = dict(p=_store32(P), g=_store32(G), m=_store32(M), v=_store32(V))
    try:
        GM.compare_groups_step(before, after, np.float32(n64), group=TG, groups=groups, max_norm=GM.MAX_NORM)
    except AssertionError:
        return True
    return False


def test_comparison_accepts_the_grouped_model_stored_in_fp32():
    for case in _cases():
        assert not _rejected(None, *case), case
    assert OM.clip_adam_step64 is GM._single_step64             # the stand-in of compare_groups_step is gone again


# mutation -> cases (steps, decoupled, side) that must reject it.  A per-group norm shows wherever the global norm
# clips (each part's norm is below the whole's) ; the lr, decay-form and step mix-ups show on both sides of the clip.
_L2 = (False, False)
MUTATIONS = {
    "group0_lr_for_group1": list(_cases()),
    "per_group_norm": [c for c in _cases() if c[2] == "clipped"],
    "l2_where_decoupled": [c for c in _cases() if c[1] == (False, True)],          # group 1's decay 0.1 is the visible one
    "group0_step_for_group1": [c for c in _cases() if c[0] == (1000, 1)],
}


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_comparison_rejects_a_near_miss_of_the_grouped_step(mutation):
    missed = [c for c in MUTATIONS[mutation] if not _rejected(mutation, *c)]
    assert not missed, (mutation, missed)
    n = sum(_rejected(mutation, *c) for c in _cases())
    print(f"{mutation}: rejected in {n} of {len(list(_cases()))} cases")
    assert n >= len(MUTATIONS[mutation]) > 0


# ---------------------------------------------------------------------------------------------------------------------
# 3. ClipAdam's constructor and add_param_group, on CPU tensors
# ---------------------------------------------------------------------------------------------------------------------
def _params(n):
    return [torch.nn.Parameter(torch.zeros(3)) for _ in range(n)]


def test_two_groups_are_accepted_with_their_own_keys():
    from wf3d.optim import ClipAdam
    a, b = _params(2)
    opt = ClipAdam([dict(params=[a], lr=1e-4), dict(params=[b], weight_decay=0.0, decoupled_weight_decay=True, betas=(0.5, 0.9))],
                   lr=1e-3, weight_decay=1e-2, max_norm=1.0)
    g0, g1 = opt.param_groups
    assert (g0["lr"], g0["weight_decay"], g0["decoupled_weight_decay"], g0["betas"]) == (1e-4, 1e-2, False, (0.9, 0.999))
    assert (g1["lr"], g1["weight_decay"], g1["decoupled_weight_decay"], g1["betas"]) == (1e-3, 0.0, True, (0.5, 0.9))
    assert ClipAdam([a], decoupled_weight_decay=True).param_groups[0]["decoupled_weight_decay"] is True
    sd = opt.state_dict()
    assert [g["lr"] for g in sd["param_groups"]] == [1e-4, 1e-3]
    opt.load_state_dict(sd)
    assert [g["decoupled_weight_decay"] for g in opt.param_groups] == [False, True]
    ref = torch.optim.Adam([dict(params=[a], lr=0.5), dict(params=[b])])
    opt.load_state_dict(ref.state_dict())                       # torch's names: the groups round-trip one by one
    assert opt.param_groups[0]["lr"] == 0.5 and all(g["capturable"] is False for g in opt.param_groups)


def test_sixteen_groups_are_the_limit():
    from wf3d.optim import ClipAdam
    ps = _params(17)
    opt = ClipAdam([dict(params=[q]) for q in ps[:16]])
    assert len(opt.param_groups) == 16
    with pytest.raises(ValueError, match="16 parameter groups"):
        opt.add_param_group(dict(params=[ps[16]]))
    assert len(opt.param_groups) == 16
    with pytest.raises(ValueError, match="16 parameter groups"):
        ClipAdam([dict(params=[q]) for q in ps])


def test_skip_nonfinite_needs_capturable():
    from wf3d.optim import ClipAdam
    with pytest.raises(ValueError, match="capturable=True"):
        ClipAdam(_params(1), skip_nonfinite=True)
    with pytest.raises(TypeError, match="skip_nonfinite"):
        ClipAdam(_params(1), capturable=True, skip_nonfinite=1)
    opt = ClipAdam(_params(1), capturable=True, skip_nonfinite=True)
    assert opt.skip_nonfinite is True and opt.skipped_steps is None          # created on the device by the first step


def test_add_param_group_is_accepted_and_validated():
    from wf3d.optim import ClipAdam
    a, b, c = _params(3)
    opt = ClipAdam([a], lr=1e-3, weight_decay=1e-6)
    opt.add_param_group(dict(params=[b], lr=1e-2, decoupled_weight_decay=True))
    assert len(opt.param_groups) == 2 and opt.param_groups[1]["lr"] == 1e-2 and opt.param_groups[1]["weight_decay"] == 1e-6
    assert opt.param_groups[1]["capturable"] is False
    with pytest.raises(ValueError, match="hyper-parameters"):
        opt.add_param_group(dict(params=[c], betas=(1.0, 0.999)))
    with pytest.raises(ValueError, match="more than one parameter group"):
        opt.add_param_group(dict(params=[a]))
    assert len(opt.param_groups) == 2                           # a refused group leaves no trace


def test_a_group_tensor_lr_needs_capturable():
    from wf3d.optim import ClipAdam
    a, b = _params(2)
    lr = torch.tensor(1e-3)
    with pytest.raises(ValueError, match="capturable=True"):
        ClipAdam([dict(params=[a]), dict(params=[b], lr=lr)])
    opt = ClipAdam([a])
    with pytest.raises(ValueError, match="capturable=True"):
        opt.add_param_group(dict(params=[b], lr=lr))
    assert len(opt.param_groups) == 1
    opt = ClipAdam([dict(params=[a]), dict(params=[b], lr=lr)], capturable=True)
    assert opt.param_groups[1]["lr"] is lr and opt.param_groups[0]["lr"] == 1e-3
    with pytest.raises(ValueError, match="0-d fp32"):
        ClipAdam([dict(params=[a]), dict(params=[b], lr=torch.tensor([1e-3]))], capturable=True)


def test_the_grouped_entry_point_checks_its_arguments():
    """Argument checks only: nothing is launched."""
    import ctypes
    from wf3d import _lib
    lib = _lib.load()
    vp = ctypes.c_void_p
    assert _lib.SIGNATURES["wf3d_clip_adam_step_groups"] == (ctypes.c_int, [vp] * 7 + [ctypes.c_int] + [vp] * 8 + [
        ctypes.c_int, ctypes.c_double, ctypes.c_int, vp, vp, ctypes.c_size_t, vp, vp])

    def call(ngroups, group, flags=0, steps=None, skipped=None, norm=None):
        n = len(group)
        tab = (vp * n)(*[0x1000] * n)                          # never dereferenced: the checks come first
        d = (ctypes.c_double * max(ngroups, 1))(*[0.5] * max(ngroups, 1))
        i = (ctypes.c_int * max(ngroups, 1))(*[1] * max(ngroups, 1))
        return lib.wf3d_clip_adam_step_groups(tab, tab, tab, tab, (ctypes.c_long * n)(*[4] * n), (ctypes.c_int * n)(*group),
                                              steps and tab, n, d, None, d, d, d, d, i, i, ngroups, 1.0, flags, skipped, None, 0,
                                              norm, None)
    E = _lib.DEFINES
    assert call(17, [0]) == E["WF3D_ERR_UNSUPPORTED"] and b"17 parameter groups" in lib.wf3d_last_error()
    assert call(2, [0, 2]) == E["WF3D_ERR_ARG"] and b"group 2 of 2" in lib.wf3d_last_error()
    assert call(2, [0, -1]) == E["WF3D_ERR_ARG"] and b"group -1 of 2" in lib.wf3d_last_error()
    assert call(2, [0, 1], flags=E["WF3D_ADAM_SKIP_NONFINITE"]) == E["WF3D_ERR_ARG"] and b"device step counters" in lib.wf3d_last_error()
    assert call(2, [0, 1], flags=2) == E["WF3D_ERR_ARG"] and b"unknown flags" in lib.wf3d_last_error()
    assert call(2, [0, 1]) == E["WF3D_ERR_WS"]                  # past every argument check, stopped before the first launch
