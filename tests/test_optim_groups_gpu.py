"""The grouped form of csrc/optim.hip (clip_adam_kernel over its GroupedTab, step_advance_finite_kernel, through
wf3d_clip_adam_step_groups and wf3d.optim.ClipAdam with parameter groups) against the float64 model
tests/optim_groups_model.py, which tests/test_optim_groups_model.py pins to torch's clip_grad_norm_ + two-group Adam /
AdamW in float64 and shows to reject near misses (another group's lr or step, a per-group norm, L2 for decoupled).

Bounds: optim_model.compare_step's own (norm 1e-5 relative; g bit-equal where the step does not clip, else elem_err <=
2e-6 under the kernel's norm; both moments 2e-6; the UPDATE p' - p within 2e-6 of max(|dp64|, rms) plus the one rounding
of the stored parameter), applied with the grouped model (optim_groups_model.compare_groups_step).  Every case keeps its
norm a factor 4 off max_norm.

Shapes: optim_model.HYPER_SIZES = 1023, 16385 and 5 elements plus a clip-only tensor of 255 — a chunk boundary, a tail,
a length that is no multiple of 4 — with 1023 and 5 in group 0 and 16385 in group 1, so that the group index is not
monotonic in table order.  Tensors are views into one flat buffer per role with poison between them, as in
tests/test_optim_forms_gpu.py (whose Flat this file uses): aligned, and with the four roles at different offsets from a
16-byte boundary.

Each case prints its worst value of every quantity (pytest -s); DESIGN.md section 5b quotes the largest."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import helpers as H  # noqa: E402,F401
import optim_groups_model as GM  # noqa: E402
import optim_model as OM  # noqa: E402
from test_optim_forms_gpu import Flat, dev  # noqa: E402

WORST = {}              # quantity -> (value, case), over the file
ALIGNED = [(0, 0, 0, 0), (0, 0, 0, 0), (0, 0, 0, 0), 0]
SHIFTED = [(1, 2, 3, 0), (3, 0, 1, 2), (2, 3, 0, 1), 1]        # p, g, m, v of each tensor at different offsets
LAYOUTS = {"aligned": ALIGNED, "shifted": SHIFTED}


def _report(label, worst):
    print(f"[optim groups] {label}: " + "  ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for k, v in worst.items():
        if v >= WORST.get(k, (-1.0, ""))[0]:
            WORST[k] = (v, label)


def _bits_equal(a, b):
    return (a is None and b is None) or np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


class GroupRig:
    """Optimised tensors `sizes` in the groups `tensor_group` (then clip-only tensors `clip_only`) as views with per-role
    offsets, a ClipAdam over them with `rows[k]` as group k's hyper-parameters (optim_groups_model.group_hp rows; their
    `step` is not used) and its state set by hand; step(): run one step and hold it to the grouped model.
    lr_tensor: the groups whose lr is a device scalar.  groups_in_opt: build the optimizer with these groups only (the
    others join through join())."""

    def __init__(self, sizes, tensor_group, clip_only=(), offs=None, *, rows, capturable=False, lr_tensor=(), skip=False,
                 groups_in_opt=None):
        from wf3d.optim import ClipAdam
        self.sizes, self.clip_only, self.tensor_group = list(sizes), list(clip_only), list(tensor_group)
        n_own = len(self.sizes)
        offs = list(offs) if offs is not None else [(0, 0, 0, 0)] * n_own + [0] * len(self.clip_only)
        offs = [o if isinstance(o, tuple) else (None, o, None, None) for o in offs]
        assert len(offs) == n_own + len(self.clip_only) and all(o[0] is None for o in offs[n_own:])
        all_sizes = self.sizes + self.clip_only
        self.flat = {r: Flat(all_sizes, [o[i] for o in offs]) for i, r in enumerate("pgmv")}
        self.rows, self.capturable = [dict(r) for r in rows], capturable
        self.params = [torch.nn.Parameter(v) for v in self.flat["p"].views[:n_own]]
        self.lazy = [torch.nn.Parameter(torch.zeros(n, device=dev())) for n in self.clip_only]
        for q, v in zip(self.params + self.lazy, self.flat["g"].views):
            q.grad = v
        self.lr = {k: torch.tensor(self.rows[k]["lr"], dtype=torch.float32, device=dev()) for k in lr_tensor}
        for k in lr_tensor:
            self.rows[k]["lr"] = float(np.float32(self.rows[k]["lr"]))
        self.in_opt = list(range(len(rows))) if groups_in_opt is None else list(groups_in_opt)
        self.opt = ClipAdam([self._group(k) for k in self.in_opt], max_norm=GM.MAX_NORM,
                            norm_params=lambda: self.params + self.lazy, capturable=capturable, skip_nonfinite=skip)
        for k in self.in_opt:
            self._set_state(k)

    def _group(self, k):
        r = self.rows[k]
        return dict(params=[q for q, t in zip(self.params, self.tensor_group) if t == k], lr=self.lr.get(k, r["lr"]),
                    betas=r["betas"], eps=r["eps"], weight_decay=r["weight_decay"], decoupled_weight_decay=r["decoupled"])

    def _set_state(self, k):
        for q, t, m, v in zip(self.params, self.tensor_group, self.flat["m"].views, self.flat["v"].views):
            if t == k:
                step = torch.zeros((), dtype=torch.float32, device=dev()) if self.capturable else torch.tensor(0.0)
                self.opt.state[q] = {"step": step, "exp_avg": m, "exp_avg_sq": v}

    def join(self, k):
        """Group k enters through add_param_group, without state: its first step creates it."""
        self.opt.add_param_group(self._group(k))
        self.in_opt.append(k)

    def load(self, before, steps):
        """Inputs of the next step; the counters of group k's tensors are set to steps[k] - 1."""
        for r in "pgmv":
            self.flat[r].write(before[r])
        for q, t in zip(self.params, self.tensor_group):
            if t in self.in_opt:
                self.opt.state[q]["step"].fill_(float(steps[t] - 1))

    def counters(self):
        """Per optimised tensor: its counter, -1 where it has no state yet."""
        where = dev() if self.capturable else torch.device("cpu")
        s = [self.opt.state[q]["step"].reshape(()).float() if self.opt.state.get(q) else torch.tensor(-1.0, device=where)
             for q in self.params]
        return torch.stack(s).cpu().numpy()

    def snapshot(self):
        snap = {r: self.flat[r].read() for r in "pgmv"}
        for i, q in enumerate(self.params):                     # moments that a step created live outside the flat buffers
            st = self.opt.state.get(q)
            if st and st["exp_avg"].data_ptr() != self.flat["m"].views[i].data_ptr():
                snap["m"][i], snap["v"][i] = st["exp_avg"].cpu().numpy(), st["exp_avg_sq"].cpu().numpy()
        return snap

    def model_view(self, snap):
        """The snapshot as the model sees it: a tensor whose group is not in the optimizer is a clip-only one."""
        tg = [t if t in self.in_opt else None for t in self.tensor_group] + [None] * len(self.clip_only)
        out = {r: [x if (r == "g" or t is not None) else None for x, t in zip(snap[r], tg)] for r in "pgmv"}
        return out, tg

    def step(self, label, before=None, *, report=True):
        """One opt.step() from the buffers as they are, compared with the grouped model at the steps the counters held + 1."""
        full_before = before or self.snapshot()
        c0 = self.counters()
        c0 = np.where(c0 < 0, 0.0, c0)                          # no state yet: the step creates it at 0
        groups = []
        for k, r in enumerate(self.rows):
            ck = {float(c) for c, t in zip(c0, self.tensor_group) if t == k}
            assert len(ck) <= 1
            groups.append(dict(r, step=int(ck.pop()) + 1 if ck else 1))
        self.opt.step()
        torch.cuda.synchronize()
        full_after = self.snapshot()
        c1 = self.counters()
        live = np.array([t in self.in_opt for t in self.tensor_group], dtype=bool)
        assert (c1[live] == c0[live] + 1.0).all(), "every step counter of a stepped tensor advances by exactly 1"
        norm = self.opt.last_grad_norm
        assert norm.shape == () and norm.dtype == torch.float32
        (b, tg), (a, _) = self.model_view(full_before), self.model_view(full_after)
        for r in "pmv":                                         # what the optimizer does not own, it does not touch
            for x, y, t in zip(full_before[r], full_after[r], tg):
                assert t is not None or _bits_equal(x, y), r
        worst = GM.compare_groups_step(b, a, np.float32(norm.item()), group=tg, groups=groups, max_norm=GM.MAX_NORM)
        if report:
            _report(label, worst)
        return full_before, full_after, worst


def _rig(layout="aligned", **kw):
    rows = kw.pop("rows", None) or GM.two_groups((1, 1), kw.pop("decoupled", (False, False)))
    return GroupRig(OM.HYPER_SIZES, GM.TENSOR_GROUP, OM.HYPER_CLIP_ONLY, LAYOUTS[layout], rows=rows, **kw)


def _inputs(steps, seed, side):
    return GM.make_group_inputs(OM.HYPER_SIZES, OM.HYPER_CLIP_ONLY, GM.TENSOR_GROUP, steps, seed=seed,
                                norm=OM.SIDES[side] * GM.MAX_NORM)


def _fresh_grads(rig, seed, norm):
    g = OM.make_inputs(rig.sizes, rig.clip_only, seed=seed, step=1, norm=norm, max_norm=GM.MAX_NORM)["g"]
    rig.flat["g"].write(g)


# ---------------------------------------------------------------------------------------------------------------------
# 1. two groups, every hyper-parameter different, both forms, groups at the same and at different steps
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("side", sorted(OM.SIDES))
@pytest.mark.parametrize("steps", GM.GROUP_STEPS)
@pytest.mark.parametrize("capturable", [False, True])
def test_two_groups_with_their_own_hyper_parameters_and_steps(capturable, steps, side, layout):
    rig = _rig(layout, capturable=capturable)
    seed = 1000 + 100 * GM.GROUP_STEPS.index(steps) + 10 * capturable + sorted(OM.SIDES).index(side)
    before = _inputs(steps, seed, side)
    rig.load(before, steps)
    rig.step(f"two groups capturable={capturable} t={steps} {side} {layout}", before)
    assert rig.counters().tolist() == [float(steps[t]) for t in GM.TENSOR_GROUP]


# ---------------------------------------------------------------------------------------------------------------------
# 2. decoupled decay on one group, L2 on the other
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", sorted(OM.SIDES))
@pytest.mark.parametrize("steps", [(2, 2), (1000, 1)])
@pytest.mark.parametrize("capturable", [False, True])
@pytest.mark.parametrize("decoupled", GM.DECAY_FORMS[1:])
def test_decoupled_decay_beside_l2(decoupled, capturable, steps, side):
    """The parameter of the decoupled group loses lr wd p beside the Adam step in one subtraction: the update bound holds
    with its one rounding allowance.  The L2 reading of the same step is refused where the decay is large (group 1)."""
    layout = "shifted" if capturable else "aligned"
    rig = _rig(layout, capturable=capturable, decoupled=decoupled)
    seed = 2000 + 100 * GM.DECAY_FORMS.index(decoupled) + 10 * capturable + sorted(OM.SIDES).index(side) + (5 if steps[1] == 1 else 0)
    before = _inputs(steps, seed, side)
    rig.load(before, steps)
    fb, fa, _ = rig.step(f"decoupled={decoupled} capturable={capturable} t={steps} {side}", before)
    if decoupled[1]:
        (b, tg), (a, _) = rig.model_view(fb), rig.model_view(fa)
        with pytest.raises(AssertionError):
            GM.compare_groups_step(b, a, np.float32(rig.opt.last_grad_norm.item()), group=tg,
                                   groups=GM.two_groups(steps, (False, False)), max_norm=GM.MAX_NORM)


# ---------------------------------------------------------------------------------------------------------------------
# 3. one group's lr a device tensor, the other's a float
# ---------------------------------------------------------------------------------------------------------------------
def test_one_groups_tensor_lr_filled_between_steps():
    rig = _rig("shifted", capturable=True, lr_tensor=(1,))
    assert torch.is_tensor(rig.opt.param_groups[1]["lr"]) and not torch.is_tensor(rig.opt.param_groups[0]["lr"])
    before = _inputs((1, 1), 3000, "clipped")
    rig.load(before, (1, 1))
    rig.step("group 1 tensor lr t=1", before)
    rig.lr[1].fill_(2.5e-3)
    old = [dict(r) for r in rig.rows]
    rig.rows[1]["lr"] = float(np.float32(2.5e-3))
    _fresh_grads(rig, 3001, 0.25)
    fb, fa, _ = rig.step("group 1 tensor lr t=2 after fill_")
    (b, tg), (a, _) = rig.model_view(fb), rig.model_view(fa)
    with pytest.raises(AssertionError):                         # and the old lr does not describe that step
        GM.compare_groups_step(b, a, np.float32(rig.opt.last_grad_norm.item()), group=tg,
                               groups=[dict(r, step=2) for r in old], max_norm=GM.MAX_NORM)


# ---------------------------------------------------------------------------------------------------------------------
# 4. two groups with the same hyper-parameters are one group, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", OM.STEPS)
@pytest.mark.parametrize("capturable", [False, True])
def test_two_equal_groups_give_the_bits_of_one_group(capturable, step):
    """The single group runs the single-group kernels (wf3d_clip_adam_step / _dev), the two groups the grouped one:
    same partial sums at the same places, same expression."""
    row = GM.group_hp(**GM.TWO_GROUPS[0])
    before = _inputs((step, step), 4000 + step, "clipped")
    out = []
    for rows, tensor_group in (([row], (0, 0, 0)), ([row, row], GM.TENSOR_GROUP)):
        rig = GroupRig(OM.HYPER_SIZES, tensor_group, OM.HYPER_CLIP_ONLY, SHIFTED[:2] + ALIGNED[2:], rows=rows, capturable=capturable)
        rig.load(before, (step, step))
        _, after, _ = rig.step(f"equal groups: {len(rows)} capturable={capturable} t={step}", before, report=False)
        out.append((after, rig.opt.last_grad_norm.item()))
    (a, na), (b, nb) = out
    assert na == nb
    for r in "pgmv":
        for x, y in zip(a[r], b[r]):
            assert _bits_equal(x, y), r


# ---------------------------------------------------------------------------------------------------------------------
# 5. many small tensors: every launch split, and the counter-advance batches
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count,skip", [(83, False), (300, True)])
def test_many_small_tensors_over_two_groups(count, skip):
    """83 tensors of 3 elements, alternating between the groups, and a clip-only one: the grouped launches split after
    48 tensors, the sum-of-squares launches after 80, and every tensor is compared under the one reported norm.  300 with
    the skip flag: two batches of the guarded counter advance (256 + 44), of which only the first counts a skip."""
    sizes, tg = [3] * count, [i % 2 for i in range(count)]
    rig = GroupRig(sizes, tg, [9], rows=GM.two_groups((1, 1)), capturable=True, skip=skip)
    before = GM.make_group_inputs(sizes, [9], tg, (3, 1), seed=5000 + count, norm=4.0)
    rig.load(before, (3, 1))
    rig.step(f"{count} small tensors t=(3, 1)", before)
    _fresh_grads(rig, 5001 + count, 0.25)
    rig.step(f"{count} small tensors t=(4, 2)")
    c = rig.counters()
    assert c.shape == (count,) and c.tolist() == [4.0, 2.0] * (count // 2) + [4.0] * (count % 2)
    if skip:
        assert rig.opt.skipped_steps.item() == 0


@pytest.mark.parametrize("capturable", [False, True])
def test_the_two_table_cuts_give_the_same_bits(capturable):
    """82 tensors of 3 elements, one of 16385 (two chunks) among the first 48 and a clip-only one of 9, at Adam step 2
    with a clipped norm.  One group: the single-group entry points, whose table is cut after 80 tensors; two groups with
    equal hyper-parameters and alternating membership: the grouped one, cut after 48.  Neither the number nor the place
    of a partial sum depends on the cut, and the update is one expression: p, g, m, v of every tensor and the reported
    norm are bit-equal."""
    sizes = [3] * 82
    sizes.insert(7, 16385)
    alternating = [i % 2 for i in range(len(sizes))]
    row = GM.group_hp(**GM.TWO_GROUPS[0])
    before = GM.make_group_inputs(sizes, [9], alternating, (2, 2), seed=5500 + capturable, norm=4.0 * GM.MAX_NORM)
    out = []
    for rows, tg in (([row], [0] * len(sizes)), ([row, row], alternating)):
        rig = GroupRig(sizes, tg, [9], rows=rows, capturable=capturable)
        rig.load(before, (2, 2))
        _, after, _ = rig.step(f"table cuts: {len(rows)} group(s) capturable={capturable}", before, report=False)
        assert rig.counters().tolist() == [2.0] * len(sizes)
        out.append((after, rig.opt.last_grad_norm.cpu().numpy()))
    (a, na), (b, nb) = out
    assert na > 2.0 * GM.MAX_NORM and _bits_equal(na, nb)
    for r in "pgmv":
        assert len(a[r]) == len(b[r]) == len(sizes) + 1
        for x, y in zip(a[r], b[r]):
            assert _bits_equal(x, y), r


# ---------------------------------------------------------------------------------------------------------------------
# 6. a group that joins after a step
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capturable", [False, True])
def test_a_group_added_after_one_step_starts_at_step_one(capturable):
    rig = _rig("aligned", capturable=capturable, groups_in_opt=[0])
    before = _inputs((1, 1), 6000 + capturable, "clipped")
    rig.load(before, (1, 1))
    _, after, _ = rig.step(f"before the second group joins capturable={capturable}", before)
    assert rig.counters().tolist() == [1.0, -1.0, 1.0]
    assert _bits_equal(after["p"][1], before["p"][1]) and not _bits_equal(after["g"][1], before["g"][1])   # clipped, not stepped
    rig.join(1)
    assert len(rig.opt.param_groups) == 2
    _fresh_grads(rig, 6002 + capturable, 4.0)
    rig.step(f"after the second group joined capturable={capturable}")
    assert rig.counters().tolist() == [2.0, 1.0, 2.0]
    q = rig.params[1]
    assert rig.opt.state[q]["exp_avg"].data_ptr() != rig.flat["m"].views[1].data_ptr()     # its state was made by the step
    _fresh_grads(rig, 6004 + capturable, 0.25)
    rig.opt.step()
    assert rig.counters().tolist() == [3.0, 2.0, 3.0]


def test_host_form_names_the_group_whose_tensors_are_at_different_steps():
    rig = _rig("aligned")
    rig.load(_inputs((2, 2), 6100, "clipped"), (2, 2))
    rig.opt.state[rig.params[2]]["step"].fill_(5.0)             # group 0: 1023 at step 2, 5 at step 6
    before = rig.snapshot()
    with pytest.raises(RuntimeError, match="group 0 are at different Adam steps"):
        rig.opt.step()
    torch.cuda.synchronize()
    after = rig.snapshot()
    for r in "pgmv":
        assert all(_bits_equal(x, y) for x, y in zip(before[r], after[r])), r


# ---------------------------------------------------------------------------------------------------------------------
# 7. the non-finite skip
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["nan_in_clip_only", "inf_in_optimised"])
def test_a_non_finite_norm_skips_the_step(where):
    rig = _rig("shifted", capturable=True, skip=True, decoupled=(False, True))
    before = _inputs((3, 7), 7000, "clipped")
    if where == "nan_in_clip_only":
        before["g"][3][200] = np.float32("nan")
    else:
        before["g"][1][16384] = np.float32(math.inf)            # the lone element of the second chunk
    rig.load(before, (3, 7))
    rig.opt.step()
    torch.cuda.synchronize()
    after = rig.snapshot()
    for r in "pgmv":                                            # nothing written: the NaN / inf is still in its place
        assert all(_bits_equal(x, y) for x, y in zip(before[r], after[r])), r
    assert rig.counters().tolist() == [2.0, 6.0, 2.0]
    assert rig.opt.skipped_steps.dtype == torch.int64 and rig.opt.skipped_steps.item() == 1
    n = rig.opt.last_grad_norm.item()
    assert math.isnan(n) if where == "nan_in_clip_only" else n == math.inf
    _fresh_grads(rig, 7001, 4.0)
    rig.step(f"the step after a skipped one ({where})")         # at counter + 1: steps 3 and 7
    assert rig.counters().tolist() == [3.0, 7.0, 3.0]
    assert rig.opt.skipped_steps.item() == 1


def test_without_the_flag_a_nan_poisons_every_group():
    rig = _rig("aligned", capturable=True)
    before = _inputs((2, 2), 7100, "unclipped")
    before["g"][3][0] = np.float32("nan")
    rig.load(before, (2, 2))
    _, after, _ = rig.step("NaN without the skip flag", before)
    assert math.isnan(rig.opt.last_grad_norm.item()) and rig.opt.skipped_steps is None
    for r in "pgmv":
        assert all(a is None or np.isnan(a).all() for a in after[r]), r


# ---------------------------------------------------------------------------------------------------------------------
# 8. captured replays
# ---------------------------------------------------------------------------------------------------------------------
def test_three_captured_replays_equal_three_eager_steps():
    """Two groups, group 1's lr a device scalar, the skip flag: warm-up step, capture of (load gradients, step), then
    three replays with new gradients and lr, the second with a NaN gradient, against the same steps run eagerly from
    the same state: tensors, counters, skipped_steps and the reported norms bit-equal."""
    from wf3d.optim import ClipAdam
    ins = _inputs((1, 1), 8000, "clipped")
    grads = [[torch.from_numpy(g).to(dev()) for g in OM.make_inputs(OM.HYPER_SIZES, [], seed=8001 + k, step=1, norm=nm, max_norm=1.0)["g"]]
             for k, nm in enumerate((4.0, 0.25, 4.0, 0.25))]
    grads[2][1][77] = float("nan")
    lrs = (1e-2, 5e-3, 2e-3, 1e-3)

    def make():
        ps = [torch.nn.Parameter(torch.from_numpy(p).to(dev())) for p in ins["p"][:3]]
        for p in ps:
            p.grad = torch.zeros_like(p)
        lr = torch.tensor(1e-2, dtype=torch.float32, device=dev())
        g0, g1 = ({k: v for k, v in r.items()} for r in GM.TWO_GROUPS)
        opt = ClipAdam([dict(g0, params=[ps[0], ps[2]]), dict(g1, params=[ps[1]], lr=lr, decoupled_weight_decay=True)],
                       max_norm=GM.MAX_NORM, capturable=True, skip_nonfinite=True)
        return ps, opt, lr, [torch.zeros_like(p) for p in ps]

    (pg, og, lrg, sg), (pe, oe, lre, se) = make(), make()

    def load_and_step(ps, opt, staged):
        for p, g in zip(ps, staged):
            p.grad.copy_(g)
        opt.step()

    def stage(staged, lr, k):
        for s, g in zip(staged, grads[k]):
            s.copy_(g)
        lr.fill_(lrs[k])

    stage(sg, lrg, 0)
    stage(se, lre, 0)
    s = torch.cuda.Stream(dev())
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        load_and_step(pg, og, sg)                               # warm-up: creates the state and skipped_steps
    torch.cuda.current_stream().wait_stream(s)
    load_and_step(pe, oe, se)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        load_and_step(pg, og, sg)
    norms = []
    for k in (1, 2, 3):
        stage(sg, lrg, k)
        graph.replay()
        norms.append(og.last_grad_norm.clone())
        stage(se, lre, k)
        load_and_step(pe, oe, se)
        assert torch.equal(norms[-1], oe.last_grad_norm) or (k == 2 and torch.isnan(norms[-1]) and torch.isnan(oe.last_grad_norm))
    torch.cuda.synchronize()
    assert round(float(norms[0]), 3) == 0.25 and math.isnan(float(norms[1])) and round(float(norms[2]), 3) == 0.25
    assert og.skipped_steps.item() == 1 == oe.skipped_steps.item()
    for a, b in zip(pg, pe):
        assert torch.equal(a, b) and torch.equal(a.grad, b.grad) and torch.isfinite(a).all()
        for key in ("exp_avg", "exp_avg_sq", "step"):
            assert torch.equal(og.state[a][key], oe.state[b][key]), key
        assert float(og.state[a]["step"]) == 3.0               # warm-up + two replays; the NaN replay advanced nothing


def test_zz_report_the_largest_errors_of_this_file():
    """Prints the maxima over the cases above (they run first in file order); asserts nothing new."""
    for k, (v, label) in sorted(WORST.items()):
        print(f"[optim groups] LARGEST {k}: {v:.3e}  ({label})")
    assert all(v <= (1.0 if k == "dp_bound" else OM.NORM_TOL if k == "norm" else OM.TOL) for k, (v, _) in WORST.items())
