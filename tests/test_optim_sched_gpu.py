"""Learning-rate schedules and averaged weights of the step tail on the device (csrc/optim.hip: lr_schedule_kernel,
clip_adam_kernel over its EmaTab, the schedule count in the step-advance kernels, ema_swap_kernel; wf3d.optim.ClipAdam with
`lr_schedule` / `ema_decay`) against tests/optim_sched_model.py, which tests/test_optim_sched_model.py pins to torch's
schedulers and EMA and shows to reject near misses.

Bounds.  p, g, m, v and the norm: optim_model.compare_step's own (TOL = 2e-6, NORM_TOL = 1e-5), through
optim_groups_model.compare_groups_step, at the rate the step reports.  The rate: float32(lr * lr_factor(schedule, t)) or
one of its two fp32 neighbours — the device's cos / pow in double may differ from the host's in the last bit of the
double, which after the one rounding is at most one fp32 ulp (derived, not measured); bit-equal in the host form and
wherever the factor is dyadic.  The average: from the kernel's own stored p',
|ema' - ema_step64| <= 2^-23 (|ema'| + 2 (1 - d) |p' - ema|) — two roundings in the product term and one in the fma,
2^-24 relative each, with a factor 2 of margin.  Everything that is claimed to be "the same step" is compared bit for bit.

Shapes: optim_model.HYPER_SIZES = 1023, 16385 and 5 elements plus a clip-only tensor of 255, as views into one flat
buffer per role (tests/test_optim_forms_gpu.py's Flat) with poison between them, the average being a fifth role at its
own offset: aligned, shifted (every role of a tensor at another offset from a 16-byte boundary), and p, g, m, v
aligned with only the average off (the f32x4 path needs all five).

Each case prints its worst value of every quantity (pytest -s); DESIGN.md section 5b quotes the largest."""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import helpers as H  # noqa: E402,F401
import optim_groups_model as GM  # noqa: E402
import optim_model as OM  # noqa: E402
import optim_sched_model as SM  # noqa: E402
from test_optim_forms_gpu import Flat, dev  # noqa: E402

WORST = {}              # quantity -> (value, case), over the file
LAYOUTS = {"aligned": [(0, 0, 0, 0, 0), (0, 0, 0, 0, 0), (0, 0, 0, 0, 0), 0],
           "shifted": [(1, 2, 3, 0, 2), (3, 0, 1, 2, 1), (2, 3, 0, 1, 3), 1],
           "ema_off": [(0, 0, 0, 0, 1), (0, 0, 0, 0, 0), (0, 0, 0, 0, 2), 0]}
ROLES = "pgmve"
TG = list(GM.TENSOR_GROUP) + [None]
DECAY = [0.999, 0.99]
WARM_COS = dict(warmup_steps=5, warmup_start=0.01, decay="cosine", decay_steps=20, min_factor=0.01)
MULTI = dict(warmup_steps=3, warmup_start=0.5, decay="multistep", gamma=0.3, milestones=(2, 2, 9))
DYADIC = dict(warmup_steps=4, warmup_start=0.25, decay="multistep", gamma=0.5, milestones=(1, 3))


def _report(label, worst):
    print(f"[optim sched] {label}: " + "  ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for k, v in worst.items():
        if v >= WORST.get(k, (-1.0, ""))[0]:
            WORST[k] = (v, label)


def _bits_equal(a, b):
    return (a is None and b is None) or np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def _same(a, b, roles=ROLES):
    for r in roles:
        for i, (x, y) in enumerate(zip(a[r], b[r])):
            assert _bits_equal(x, y), (r, i)


class SchedRig:
    """optim_model.HYPER_SIZES in optim_groups_model.TENSOR_GROUP's two groups plus the clip-only tensor, as views with
    per-role offsets (p, g, m, v, e), a ClipAdam over them with its state set by hand, and step(): one step held to
    optim_sched_model.compare_sched_step.  ema_decay[k] None: group k keeps no average (and its tensors no fifth view)."""

    def __init__(self, layout="aligned", *, rows=None, capturable=False, skip=False, schedules=(None, None),
                 ema_decay=(None, None), ema_warmup=False, lr_tensor=False):
        from wf3d.optim import ClipAdam
        self.sizes, self.clip_only = list(OM.HYPER_SIZES), list(OM.HYPER_CLIP_ONLY)
        self.rows = [dict(r) for r in (rows or GM.two_groups((1, 1)))]
        self.capturable, self.schedules, self.ema_decay, self.ema_warmup = capturable, list(schedules), list(ema_decay), ema_warmup
        offs = [o if isinstance(o, tuple) else (None, o, None, None, None) for o in LAYOUTS[layout]]
        offs = [o if o[0] is None or self.ema_decay[k] else o[:4] + (None,) for o, k in zip(offs, TG)]
        self.flat = {r: Flat(self.sizes + self.clip_only, [o[i] for o in offs]) for i, r in enumerate(ROLES)}
        self.params = [torch.nn.Parameter(v) for v in self.flat["p"].views[:3]]
        self.lazy = [torch.nn.Parameter(torch.zeros(n, device=dev())) for n in self.clip_only]
        for q, v in zip(self.params + self.lazy, self.flat["g"].views):
            q.grad = v
        self.lr = [torch.tensor(r["lr"], dtype=torch.float32, device=dev()) for r in self.rows] if lr_tensor else None
        groups = []
        for k, r in enumerate(self.rows):
            groups.append(dict(params=[q for q, t in zip(self.params, GM.TENSOR_GROUP) if t == k], lr=self.lr[k] if lr_tensor else r["lr"],
                               betas=r["betas"], eps=r["eps"], weight_decay=r["weight_decay"], decoupled_weight_decay=r["decoupled"],
                               lr_schedule=self.schedules[k], ema_decay=self.ema_decay[k]))
        self.opt = ClipAdam(groups, max_norm=GM.MAX_NORM, norm_params=lambda: self.params + self.lazy, capturable=capturable,
                            skip_nonfinite=skip, ema_warmup=ema_warmup)
        for q, m, v, e in zip(self.params, self.flat["m"].views, self.flat["v"].views, self.flat["e"].views):
            step = torch.zeros((), dtype=torch.float32, device=dev()) if capturable else torch.tensor(0.0)
            self.opt.state[q] = {"step": step, "exp_avg": m, "exp_avg_sq": v}
            if e is not None:
                self.opt.state[q]["ema"] = e
        for q, o in zip(self.params, offs):                     # the path each tensor takes, from the pointers themselves
            st = self.opt.state[q]
            ptrs = [q.data_ptr(), q.grad.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()]
            ptrs += [st["ema"].data_ptr()] if "ema" in st else []
            assert [a % 16 for a in ptrs] == [4 * k for k in o if k is not None]

    def load(self, before, steps, t=0):
        """Inputs of the next step (optim_sched_model.add_averages' dict); group k's counters at steps[k] - 1, the count at t."""
        for r in ROLES:
            self.flat[r].write(before[r])
        for q, k in zip(self.params, GM.TENSOR_GROUP):
            self.opt.state[q]["step"].fill_(float(steps[k] - 1))
        self.opt.set_schedule_step(t)

    def counters(self):
        return torch.stack([self.opt.state[q]["step"].reshape(()).float().cpu() for q in self.params]).numpy()

    def count(self):
        return self.opt.state_dict()["schedule_step"]

    def snapshot(self):
        snap = {r: self.flat[r].read() for r in ROLES}
        snap["t"] = self.count()
        snap["lr"] = None if self.opt.last_lr is None else [float(x) for x in self.opt.last_lr.cpu()]
        return snap

    def fresh_grads(self, seed, norm):
        self.flat["g"].write(OM.make_inputs(self.sizes, self.clip_only, seed=seed, step=1, norm=norm, max_norm=GM.MAX_NORM)["g"])

    def step(self, label, before=None, *, report=True, skipped=False):
        before = before or self.snapshot()
        before = dict(before, t=self.count())
        c0 = self.counters()
        groups = [dict(r, step=int(c0[GM.TENSOR_GROUP.index(k)]) + 1) for k, r in enumerate(self.rows)]
        self.opt.step()
        torch.cuda.synchronize()
        after = self.snapshot()
        assert (self.counters() == c0 + (0.0 if skipped else 1.0)).all()
        worst = SM.compare_sched_step(before, after, np.float32(self.opt.last_grad_norm.item()), group=TG, groups=groups,
                                      max_norm=GM.MAX_NORM, schedules=self.schedules, ema_decay=self.ema_decay,
                                      ema_warmup=self.ema_warmup, skipped=skipped, lr_ulps=1 if self.capturable else 0)
        if report and worst:
            _report(label, worst)
        return before, after, worst


def _inputs(steps, seed, side, ema_decay=DECAY, t=0):
    b = GM.make_group_inputs(OM.HYPER_SIZES, OM.HYPER_CLIP_ONLY, GM.TENSOR_GROUP, steps, seed=seed, norm=OM.SIDES[side] * GM.MAX_NORM)
    return SM.add_averages(b, TG, ema_decay, seed + 1, t=t)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the applied rate
# ---------------------------------------------------------------------------------------------------------------------
def test_the_applied_rate_at_every_edge_of_two_schedules():
    from wf3d.optim import ClipAdam, lr_factor
    W, T = WARM_COS["warmup_steps"], WARM_COS["decay_steps"]
    ps = [torch.nn.Parameter(torch.full((n,), 0.02, device=dev())) for n in (5, 3)]
    lrs, schedules = (1e-3, 3e-4), (WARM_COS, MULTI)
    opt = ClipAdam([dict(params=[p], lr=lr, lr_schedule=s) for p, lr, s in zip(ps, lrs, schedules)], capturable=True, max_norm=1.0)
    equal = total = 0
    for t in (0, 1, W - 1, W, W + 1, W + T - 1, W + T, W + T + 5, 2 ** 24 + 1):
        for p in ps:
            p.grad = torch.full_like(p, 0.1)
        opt.set_schedule_step(t)
        opt.step()
        got = opt.last_lr.cpu().numpy()
        assert opt.last_lr.dtype == torch.float32 and got.shape == (2,) and opt.schedule_step.dtype == torch.int64
        assert int(opt.schedule_step) == t + 1                  # exact past 2^24, where an fp32 counter is not
        for k in range(2):
            want = np.float32(lrs[k] * lr_factor(schedules[k], t))
            print(f"[optim sched] rate t={t} group {k}: device {got[k]!r} host {want!r}")
            assert float(got[k]) in SM.neighbours32(want), (t, k, got[k], want)
            equal += int(got[k] == want)
            total += 1
    print(f"[optim sched] applied rate: {equal} of {total} entries bit-equal to float32(lr * lr_factor)")
    assert [g["lr"] for g in opt.param_groups] == list(lrs)    # the base rate stays what it was


# ---------------------------------------------------------------------------------------------------------------------
# 2. the schedule changes nothing but the rate
# ---------------------------------------------------------------------------------------------------------------------
def test_a_scheduled_step_is_the_unscheduled_step_at_the_reported_rate():
    """Six steps of a scheduled optimizer against an optimizer without schedule whose tensor lr is copied from the
    rates the first one reports: p, g, m, v, counters and norm bit for bit (wf3d_clip_adam_step_groups' kernels on
    the second side).  The first also reports a group without schedule at its base rate."""
    a = SchedRig("shifted", capturable=True, schedules=(WARM_COS, MULTI))
    b = SchedRig("shifted", capturable=True, lr_tensor=True)
    before = _inputs((1, 1), 2000, "clipped", ema_decay=(None, None))
    a.load(before, (1, 1), t=3)
    b.load(before, (1, 1))
    seen = []
    for k in range(6):
        for rig in (a, b):
            rig.fresh_grads(2001 + k, (4.0, 0.25)[k % 2])
        _, sa, _ = a.step(f"scheduled t={3 + k}")
        for lr, x in zip(b.lr, a.opt.last_lr):
            lr.copy_(x)
        b.opt.step()
        torch.cuda.synchronize()
        sb = b.snapshot()
        _same(sa, sb, "pgmv")
        assert np.array_equal(a.counters(), b.counters()) and torch.equal(a.opt.last_grad_norm, b.opt.last_grad_norm)
        seen.append(tuple(sa["lr"]))
    assert a.count() == 9 and b.opt.last_lr is None and len(set(seen)) == 6
    c = SchedRig("aligned", capturable=True, schedules=(None, MULTI))
    c.load(before, (1, 1))
    _, sc, _ = c.step("one group without schedule")
    assert sc["lr"][0] == float(np.float32(GM.TWO_GROUPS[0]["lr"]))


def test_a_tensor_lr_beside_a_scheduled_group_keeps_its_tensor():
    from wf3d.optim import ClipAdam
    ps = [torch.nn.Parameter(torch.full((n,), 0.02, device=dev())) for n in (5, 3)]
    lr = torch.tensor(2e-3, device=dev())
    opt = ClipAdam([dict(params=[ps[0]], lr=lr), dict(params=[ps[1]], lr_schedule=DYADIC)], lr=1e-3, capturable=True)
    for p in ps:
        p.grad = torch.full_like(p, 0.1)
    opt.step()
    got = opt.last_lr.cpu().numpy()
    assert math.isnan(got[0]) and got[1] == np.float32(1e-3 * 0.25)          # no write for the tensor-lr group
    first = [float(p.detach()[0]) for p in ps]
    assert first == [pytest.approx(0.02 - 2e-3, rel=1e-5), pytest.approx(0.02 - 2.5e-4, rel=1e-5)]


# ---------------------------------------------------------------------------------------------------------------------
# 3. host and device forms agree
# ---------------------------------------------------------------------------------------------------------------------
def test_host_and_capturable_forms_agree_on_a_dyadic_schedule():
    """warm-up 4 from 0.25, multistep gamma 0.5: every factor is exact in double, so both forms round the same product."""
    rigs = [SchedRig("aligned", capturable=c, schedules=(DYADIC, DYADIC), ema_decay=DECAY, ema_warmup=True) for c in (False, True)]
    before = _inputs((1, 1), 3000, "clipped")
    for rig in rigs:
        rig.load(before, (1, 1))
    for k in range(8):
        snaps = []
        for rig in rigs:
            rig.fresh_grads(3001 + k, (4.0, 0.25)[k % 2])
            snaps.append(rig.step(f"dyadic t={k} capturable={rig.capturable}", report=False)[1])
        _same(*snaps)
        assert snaps[0]["lr"] == snaps[1]["lr"] and snaps[0]["t"] == snaps[1]["t"] == k + 1
        assert np.array_equal(rigs[0].counters(), rigs[1].counters())
    assert rigs[0].opt.last_lr.device.type == "cpu" and rigs[1].opt.last_lr.is_cuda and isinstance(rigs[0].opt.schedule_step, int)


# ---------------------------------------------------------------------------------------------------------------------
# 4. EMA against the model
# ---------------------------------------------------------------------------------------------------------------------
FORMS = [(dec, warm, cap) for dec in (False, True) for warm in (False, True) for cap in (False, True)]


@pytest.mark.parametrize("side", sorted(OM.SIDES))
@pytest.mark.parametrize("step", OM.STEPS)
@pytest.mark.parametrize("decoupled,warmup,capturable", FORMS)
def test_the_average_follows_the_stored_parameter(decoupled, warmup, capturable, step, side):
    """Every (decay form, warm-up, host / capturable) at Adam steps 1, 2 and 1000 on both sides of the clip; the layout
    alternates so that each of the three factors meets both layouts."""
    layout = "shifted" if (decoupled + warmup + capturable) % 2 else "aligned"
    rig = SchedRig(layout, rows=GM.two_groups((1, 1), (False, decoupled)), capturable=capturable, ema_decay=DECAY, ema_warmup=warmup)
    seed = 4000 + 100 * FORMS.index((decoupled, warmup, capturable)) + 10 * OM.STEPS.index(step) + sorted(OM.SIDES).index(side)
    before = _inputs((step, step), seed, side)
    rig.load(before, (step, step))
    _, after, worst = rig.step(f"ema decoupled={decoupled} warmup={warmup} capturable={capturable} t={step} {side} {layout}", before)
    assert after["lr"] is None and after["t"] == 0            # no schedule: no rates, and nothing counts
    assert all(not _bits_equal(b, a) for b, a in zip(before["e"][:3], after["e"][:3]))


def test_only_the_average_off_alignment_and_a_group_without_average():
    """p, g, m, v aligned and the average off a 16-byte boundary: the element-wise path; group 1 keeps no average and its
    tensor runs the four-pointer walk inside the EMA launch.  lr = 0: the average still moves."""
    rows = GM.two_groups((1, 1))
    rows[0]["lr"] = 0.0
    rig = SchedRig("ema_off", rows=rows, capturable=True, ema_decay=(0.999, None))
    before = _inputs((2, 2), 4900, "clipped", ema_decay=(0.999, None))
    rig.load(before, (2, 2))
    _, after, _ = rig.step("ema off alignment, lr 0", before)
    assert after["e"][1] is None and "ema" not in rig.opt.state[rig.params[1]]
    for i in (0, 2):
        assert _bits_equal(before["p"][i], after["p"][i]) and not _bits_equal(before["e"][i], after["e"][i])


# ---------------------------------------------------------------------------------------------------------------------
# 5. EMA is a side output
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("capturable,skip", [(False, False), (True, False), (True, True)])
def test_the_step_with_an_average_is_the_step_without_bit_for_bit(capturable, skip, layout):
    out = []
    for decay in ((None, None), tuple(DECAY)):
        rig = SchedRig(layout, rows=GM.two_groups((1, 1), (False, True)), capturable=capturable, skip=skip, ema_decay=decay, ema_warmup=True)
        before = _inputs((2, 2), 5000, "clipped", ema_decay=decay)
        rig.load(before, (2, 2))
        for k in range(2):
            rig.fresh_grads(5001 + k, (4.0, 0.25)[k])
            rig.opt.step()
        torch.cuda.synchronize()
        out.append((rig.snapshot(), rig.counters(), rig.opt.last_grad_norm.item()))
    (a, ca, na), (b, cb, nb) = out
    _same(a, b, "pgmv")
    assert np.array_equal(ca, cb) and ca.tolist() == [3.0] * 3 and na == nb
    assert all(x is None for x in a["e"]) and all(x is not None for x in b["e"][:3])


# ---------------------------------------------------------------------------------------------------------------------
# 6. the non-finite skip
# ---------------------------------------------------------------------------------------------------------------------
def test_a_skipped_step_moves_neither_average_nor_count_nor_rate():
    rig = SchedRig("shifted", capturable=True, skip=True, schedules=(WARM_COS, MULTI), ema_decay=DECAY, ema_warmup=True)
    before = _inputs((3, 7), 6000, "clipped")
    rig.load(before, (3, 7), t=2)
    rig.step("the step before the skipped one", before)
    assert rig.count() == 3
    rate3 = [SM.applied_lr(GM.TWO_GROUPS[k]["lr"], s, 3) for k, s in enumerate((WARM_COS, MULTI))]
    rig.fresh_grads(6001, 4.0)
    g = rig.flat["g"].read()
    g[1][16384] = np.float32(math.inf)                          # the lone element of the second chunk
    rig.flat["g"].write(g)
    _, after, _ = rig.step("skipped", skipped=True)
    assert rig.opt.skipped_steps.item() == 1 and rig.count() == 3 and math.isinf(rig.opt.last_grad_norm.item())
    assert all(x in SM.neighbours32(w) for x, w in zip(after["lr"], rate3))  # the rate it would have applied
    rig.fresh_grads(6002, 0.25)
    _, after, _ = rig.step("the step after the skipped one")    # held to the factor at t = 3, the count that did not advance
    assert all(x in SM.neighbours32(w) for x, w in zip(after["lr"], rate3))
    assert rig.count() == 4 and rig.opt.skipped_steps.item() == 1 and rig.counters().tolist() == [4.0, 8.0, 4.0]


def test_a_step_of_clip_only_tensors_advances_no_count():
    rig = SchedRig("aligned", capturable=True, skip=True, schedules=(WARM_COS, MULTI), ema_decay=DECAY)
    before = _inputs((3, 3), 6100, "clipped")
    rig.load(before, (3, 3), t=5)
    rig.step("a step that creates the count", before)
    for q in rig.params:
        q.grad = None
    snap = rig.snapshot()
    rig.opt.step()
    torch.cuda.synchronize()
    after = rig.snapshot()
    _same(snap, after, "pmve")
    assert rig.count() == 6 and rig.counters().tolist() == [3.0] * 3 and rig.opt.last_grad_norm.item() > 0.0


# ---------------------------------------------------------------------------------------------------------------------
# 7. swap
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_swap_exchanges_parameters_and_averages(layout):
    rig = SchedRig(layout, capturable=True, ema_decay=(0.999, None))
    before = _inputs((2, 2), 7000, "clipped", ema_decay=(0.999, None))
    rig.load(before, (2, 2))
    versions = [q._version for q in rig.params]
    rig.opt.swap_ema()
    torch.cuda.synchronize()
    swapped = rig.snapshot()
    for i in (0, 2):
        assert _bits_equal(swapped["p"][i], before["e"][i]) and _bits_equal(swapped["e"][i], before["p"][i])
    assert _bits_equal(swapped["p"][1], before["p"][1]) and swapped["e"][1] is None     # group 1 keeps no average
    _same(before, swapped, "gmv")
    assert all(rig.params[i]._version > versions[i] for i in (0, 2))       # (the views of one buffer share one counter)
    with pytest.raises(RuntimeError, match="swapped in"):
        rig.opt.step()
    torch.cuda.synchronize()
    _same(swapped, rig.snapshot())
    rig.opt.swap_ema()
    torch.cuda.synchronize()
    _same(before, rig.snapshot())
    with rig.opt.ema_weights():
        assert torch.equal(rig.params[0].detach().cpu(), torch.from_numpy(before["e"][0]))
    torch.cuda.synchronize()
    _same(before, rig.snapshot())
    rig.step("a step after swapping back", before)
    from wf3d.optim import ClipAdam
    with pytest.raises(RuntimeError, match="before any parameter has an average"):
        ClipAdam([torch.nn.Parameter(torch.zeros(3, device=dev()))], ema_decay=0.9).swap_ema()


# ---------------------------------------------------------------------------------------------------------------------
# 8. one capture, eight replays
# ---------------------------------------------------------------------------------------------------------------------
def test_eight_captured_replays_equal_eight_eager_steps():
    """Two groups, warm-up 2 + cosine 4, averages with warm-up, the skip flag.  Warm-up step, capture of (load
    gradients, step), eight replays with fresh gradients, the third with an infinity, against a twin stepped eagerly:
    everything bit for bit, the sequence of last_lr included.  Then a swap captured in its own graph."""
    from wf3d.optim import ClipAdam
    sched = dict(warmup_steps=2, warmup_start=0.25, decay="cosine", decay_steps=4, min_factor=0.1)
    ins = GM.make_group_inputs(OM.HYPER_SIZES, [], GM.TENSOR_GROUP, (1, 1), seed=8000, norm=4.0)
    grads = [[torch.from_numpy(g).to(dev()) for g in OM.make_inputs(OM.HYPER_SIZES, [], seed=8001 + k, step=1, norm=nm, max_norm=1.0)["g"]]
             for k, nm in enumerate((4.0, 0.25) * 4 + (4.0,))]
    grads[3][1][16384] = float("inf")                           # the third replay

    def make():
        ps = [torch.nn.Parameter(torch.from_numpy(p).to(dev())) for p in ins["p"][:3]]
        for p in ps:
            p.grad = torch.zeros_like(p)
        g0, g1 = (dict(r) for r in GM.TWO_GROUPS)
        opt = ClipAdam([dict(g0, params=[ps[0], ps[2]]), dict(g1, params=[ps[1]], decoupled_weight_decay=True, ema_decay=0.99)],
                       max_norm=GM.MAX_NORM, capturable=True, skip_nonfinite=True, lr_schedule=sched, ema_decay=0.999, ema_warmup=True)
        return ps, opt, [torch.zeros_like(p) for p in ps]

    (pg, og, sg), (pe, oe, se) = make(), make()

    def load_and_step(ps, opt, staged):
        for p, g in zip(ps, staged):
            p.grad.copy_(g)
        opt.step()

    def stage(staged, k):
        for s, g in zip(staged, grads[k]):
            s.copy_(g)

    stage(sg, 0)
    stage(se, 0)
    s = torch.cuda.Stream(dev())
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        load_and_step(pg, og, sg)                               # warm-up: creates the state, the averages and the counts
    torch.cuda.current_stream().wait_stream(s)
    load_and_step(pe, oe, se)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        load_and_step(pg, og, sg)
    rates = []
    for k in range(1, 9):
        stage(sg, k)
        graph.replay()
        rates.append(og.last_lr.clone())
        stage(se, k)
        load_and_step(pe, oe, se)
        assert torch.equal(rates[-1], oe.last_lr), k
        assert torch.equal(og.last_grad_norm, oe.last_grad_norm), k
    torch.cuda.synchronize()
    assert og.skipped_steps.item() == 1 == oe.skipped_steps.item()
    assert int(og.schedule_step) == 8 == int(oe.schedule_step)  # warm-up + eight replays - one skipped
    for a, b in zip(pg, pe):
        assert torch.equal(a, b) and torch.isfinite(a).all()
        for key in ("exp_avg", "exp_avg_sq", "step", "ema"):
            assert torch.equal(og.state[a][key], oe.state[b][key]), key
        assert float(og.state[a]["step"]) == 8.0 and not torch.equal(og.state[a]["ema"], a)
    # t = 1, 2, 3, 3 (the skipped replay and the one after it apply the same rate), 4, ...: warm-up, then the cosine to its floor
    host = [[SM.applied_lr(r["lr"], sched, t) for r in GM.TWO_GROUPS] for t in (1, 2, 3, 3, 4, 5, 6, 7)]
    for got, want in zip(rates, host):
        assert all(float(x) in SM.neighbours32(w) for x, w in zip(got.cpu(), want)), (got, want)
    assert torch.equal(rates[2], rates[3]) and not torch.equal(rates[3], rates[4]) and torch.equal(rates[6], rates[7])
    p0, e0 = [p.detach().clone() for p in pg], [og.state[p]["ema"].clone() for p in pg]
    swap = torch.cuda.CUDAGraph()
    with torch.cuda.graph(swap):
        og.swap_ema()
    swap.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(p, e) for p, e in zip(pg, e0)) and all(torch.equal(og.state[p]["ema"], q) for p, q in zip(pg, p0))
    swap.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(p, q) for p, q in zip(pg, p0)) and all(torch.equal(og.state[p]["ema"], e) for p, e in zip(pg, e0))


def test_a_capture_before_the_first_scheduled_step_is_refused():
    from wf3d.optim import ClipAdam
    p = torch.nn.Parameter(torch.zeros(8, device=dev()))
    p.grad = torch.ones_like(p)
    plain = ClipAdam([p], capturable=True)
    plain.step()                                                # the state exists; the count does not
    opt = ClipAdam([p], capturable=True, lr_schedule=DYADIC)
    sd = plain.state_dict()
    sd["param_groups"][0]["lr_schedule"] = DYADIC               # the saved group's own key (None) would replace the schedule
    opt.load_state_dict(sd)
    torch.cuda.synchronize()
    x = torch.zeros(4, device=dev())
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="before the capture"):
        with torch.cuda.graph(graph):
            x.add_(1.0)
            opt.step()
    assert opt.schedule_step is None


# ---------------------------------------------------------------------------------------------------------------------
# 9. no-feature calls of the new entry point
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capturable", [False, True])
def test_the_new_entry_point_without_features_gives_the_grouped_entry_points_bits(capturable):
    from wf3d import _lib
    lib = _lib.load()
    vp = ctypes.c_void_p
    before = GM.make_group_inputs(OM.HYPER_SIZES, OM.HYPER_CLIP_ONLY, GM.TENSOR_GROUP, (2, 2), seed=9000, norm=4.0)
    n, ng = 4, 2
    dbl, integer = ctypes.c_double * ng, ctypes.c_int * ng
    out = []
    for new in (False, True):
        t = {r: [None if x is None else torch.from_numpy(x).to(dev()) for x in before[r]] for r in "pgmv"}
        steps = [torch.ones((), device=dev()) for _ in range(3)]
        norm, skipped = torch.zeros((), device=dev()), torch.zeros((), dtype=torch.int64, device=dev())
        tab = lambda xs: (vp * n)(*[None if x is None else x.data_ptr() for x in xs])      # noqa: E731
        numel = (ctypes.c_long * n)(*[g.numel() for g in t["g"]])
        nws = lib.wf3d_clip_adam_ws_floats(numel, n)
        ws = torch.empty(nws, device=dev())
        head = (tab(t["p"]), tab(t["g"]), tab(t["m"]), tab(t["v"]))
        rest = (numel, (ctypes.c_int * n)(0, 1, 0, -1), tab(steps + [None]) if capturable else None, n,
                dbl(*[r["lr"] for r in GM.TWO_GROUPS]), None, dbl(*[r["betas"][0] for r in GM.TWO_GROUPS]),
                dbl(*[r["betas"][1] for r in GM.TWO_GROUPS]), dbl(*[r["eps"] for r in GM.TWO_GROUPS]),
                dbl(*[r["weight_decay"] for r in GM.TWO_GROUPS]), integer(0, 1))
        flags = _lib.DEFINES["WF3D_ADAM_SKIP_NONFINITE"] if capturable else 0
        tail = (ng, GM.MAX_NORM, flags, skipped.data_ptr() if capturable else None)
        end = (ws.data_ptr(), nws, norm.data_ptr(), None)
        if new:
            rc = lib.wf3d_clip_adam_step_ema(*head, None, *rest, None, integer(2, 2), *tail, None, *end)
        else:
            rc = lib.wf3d_clip_adam_step_groups(*head, *rest, integer(2, 2), *tail, *end)
        assert rc == 0, lib.wf3d_last_error()
        torch.cuda.synchronize()
        out.append(({r: [None if x is None else x.cpu().numpy() for x in t[r]] for r in "pgmv"}, norm.item(),
                    [s.item() for s in steps], skipped.item()))
    (a, na, sa, ka), (b, nb, sb, kb) = out
    _same(a, b, "pgmv")
    assert na == nb and sa == sb == ([2.0] * 3 if capturable else [1.0] * 3) and ka == kb == 0
    assert not _bits_equal(a["p"][0], before["p"][0])


def test_zz_report_the_largest_errors_of_this_file():
    """Prints the maxima over the cases above (they run first in file order); asserts nothing new."""
    for k, (v, label) in sorted(WORST.items()):
        print(f"[optim sched] LARGEST {k}: {v:.3e}  ({label})")
    bound = {"dp_bound": 1.0, "e": 1.0, "norm": OM.NORM_TOL}
    assert all(v <= bound.get(k, OM.TOL) for k, (v, _) in WORST.items())
