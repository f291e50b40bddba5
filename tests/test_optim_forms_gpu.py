"""Every kernel form of csrc/optim.hip (gradsq_kernel, clip_adam_kernel, step_advance_kernel) through wf3d.optim.ClipAdam,
one step at a time from fp32 inputs, against the float64 model tests/optim_model.py (pinned to torch's clip_grad_norm_ +
Adam in float64 by tests/test_optim_model.py, which also shows that this comparison rejects subtly wrong updates).

Bounds (optim_model.compare_step): norm 1e-5 relative; g bit-equal where the step does not clip, else elem_err <= 2e-6
of the model under the kernel's own norm; both moments elem_err <= 2e-6; and the UPDATE p' - p, not the parameter,
within 2e-6 of max(|dp64|, rms(dp64)) plus the one rounding of the stored parameter.  Every case keeps its norm a factor
4 off max_norm.

Tensors are views into one flat buffer per role (p, g, m, v) at chosen offsets of 0..3 floats from a 16-byte boundary,
so that the element-wise loops run as well as the f32x4 ones; what the case claims is asserted from data_ptr().  All that
lies between the views is a poison value that must still be there after the step.

Each case prints its worst value of every quantity (pytest -s); DESIGN.md section 5b quotes the largest."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import helpers as H  # noqa: E402,F401
import optim_model as OM  # noqa: E402

GUARD = 64              # floats between views (a multiple of 4: offsets stay what the case asks for)
POISON = -12345.0
WORST = {}              # quantity -> (value, case), over the file


def dev():
    return torch.device("cuda:0")


def _report(label, worst):
    print(f"[optim forms] {label}: " + "  ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for k, v in worst.items():
        if v >= WORST.get(k, (-1.0, ""))[0]:
            WORST[k] = (v, label)


class Flat:
    """One role's flat buffer: views at offsets[i] floats past a 16-byte boundary (None: the tensor has no such role)."""

    def __init__(self, sizes, offsets):
        self.spans, cur = [], GUARD
        for n, k in zip(sizes, offsets):
            if k is None:
                self.spans.append(None)
                continue
            start = (cur + 3) // 4 * 4 + k
            self.spans.append((start, start + n))
            cur = start + n + GUARD
        self.buf = torch.full((cur + 4,), POISON, dtype=torch.float32, device=dev())
        assert self.buf.data_ptr() % 16 == 0
        self.views = [None if s is None else self.buf[s[0]:s[1]] for s in self.spans]
        for v, k in zip(self.views, offsets):
            assert v is None or (v.data_ptr() % 16 == 4 * k and v.is_contiguous())
        self.between = np.ones(cur + 4, dtype=bool)
        for s in self.spans:
            if s is not None:
                self.between[s[0]:s[1]] = False

    def write(self, arrays):
        host = np.full(self.buf.numel(), POISON, dtype=np.float32)
        for s, a in zip(self.spans, arrays):
            if s is not None:
                host[s[0]:s[1]] = a
        self.buf.copy_(torch.from_numpy(host))

    def read(self):
        """The views' values (one copy), after checking that nothing between them was written."""
        host = self.buf.cpu().numpy()
        assert (host[self.between] == np.float32(POISON)).all(), "a kernel wrote outside its tensors"
        return [None if s is None else host[s[0]:s[1]].copy() for s in self.spans]


class Rig:
    """Optimised tensors `sizes` (then clip-only tensors `clip_only`) as views with per-role offsets
    offs[i] = (kp, kg, km, kv) (clip-only: (None, kg, None, None) or just kg), a ClipAdam over them with its state set
    by hand, and step(): run one step and hold it to the model."""

    def __init__(self, sizes, clip_only=(), offs=None, *, hp, capturable=False, lr_tensor=False):
        from wf3d.optim import ClipAdam
        self.sizes, self.clip_only = list(sizes), list(clip_only)
        n_own, n_all = len(self.sizes), len(self.sizes) + len(self.clip_only)
        offs = list(offs) if offs is not None else [(0, 0, 0, 0)] * n_own + [0] * len(self.clip_only)
        offs = [o if isinstance(o, tuple) else (None, o, None, None) for o in offs]
        assert len(offs) == n_all and all(o[0] is None for o in offs[n_own:])
        self.offs, all_sizes = offs, self.sizes + self.clip_only
        self.flat = {r: Flat(all_sizes, [o[i] for o in offs]) for i, r in enumerate("pgmv")}
        self.hp, self.capturable = dict(hp), capturable
        self.params = [torch.nn.Parameter(v) for v in self.flat["p"].views[:n_own]]
        self.lazy = [torch.nn.Parameter(torch.zeros(n, device=dev())) for n in self.clip_only]
        for q, v in zip(self.params + self.lazy, self.flat["g"].views):
            q.grad = v
        self.lr = torch.tensor(hp["lr"], dtype=torch.float32, device=dev()) if lr_tensor else hp["lr"]
        self.opt = ClipAdam(self.params, lr=self.lr, betas=hp["betas"], eps=hp["eps"], weight_decay=hp["weight_decay"],
                            max_norm=hp["max_norm"], norm_params=lambda: self.params + self.lazy, capturable=capturable)
        for q, m, v in zip(self.params, self.flat["m"].views, self.flat["v"].views):
            step = torch.zeros((), dtype=torch.float32, device=dev()) if capturable else torch.tensor(0.0)
            self.opt.state[q] = {"step": step, "exp_avg": m, "exp_avg_sq": v}
        for q, o in zip(self.params + self.lazy, offs):          # the path each tensor takes, from the pointers themselves
            ptrs = [q.grad.data_ptr()] if o[0] is None else [q.data_ptr(), q.grad.data_ptr()] + \
                [self.opt.state[q][k].data_ptr() for k in ("exp_avg", "exp_avg_sq")]
            want = [o[1]] if o[0] is None else list(o)
            assert [a % 16 for a in ptrs] == [4 * k for k in want]

    def paths(self):
        """(tensors whose sum of squares runs as f32x4, as elements; whose Adam update runs as f32x4, as elements; clip-only)"""
        sq = sum(o[1] == 0 for o in self.offs)
        own = [o for o in self.offs if o[0] is not None]
        vec = sum(o == (0, 0, 0, 0) for o in own)
        return sq, len(self.offs) - sq, vec, len(own) - vec, len(self.offs) - len(own)

    def load(self, before, step):
        """Inputs of the next step: a `before` dict of optim_model.make_inputs; the counters are set to step - 1."""
        for r in "pgmv":
            self.flat[r].write(before[r])
        for q in self.params:
            self.opt.state[q]["step"].fill_(float(step - 1))

    def counters(self):
        s = [self.opt.state[q]["step"] for q in self.params]
        return torch.stack(s).cpu().numpy() if s else np.zeros(0, np.float32)

    def snapshot(self):
        return {r: self.flat[r].read() for r in "pgmv"}

    def step(self, label, before=None, *, hp=None, report=True):
        """One opt.step() from the buffers as they are, compared with the model at the step the counters held + 1."""
        before = before or self.snapshot()
        c0 = self.counters()
        assert len(set(c0.tolist())) <= 1
        t = int(c0[0]) + 1 if len(c0) else 1
        self.opt.step()
        torch.cuda.synchronize()
        after = self.snapshot()
        c1 = self.counters()
        assert (c1 == c0 + 1.0).all(), "every step counter advances by exactly 1"
        norm = self.opt.last_grad_norm
        assert norm.shape == () and norm.dtype == torch.float32
        worst = OM.compare_step(before, after, np.float32(norm.item()), step=t, **(hp or self.hp))
        if report:
            _report(label, worst)
        return before, after, worst


# ---------------------------------------------------------------------------------------------------------------------
# a. alignment x size
# ---------------------------------------------------------------------------------------------------------------------
# one tensor per row, all of the same size, stepped together: the kernels choose the form per tensor
ALIGN = ([(0, 0, 0, 0)] +                                       # f32x4 in both kernels
         [(k, 0, 0, 0) for k in (1, 2, 3)] +                    # p off: gradsq f32x4, Adam element-wise
         [(0, k, 0, 0) for k in (1, 2, 3)] +                    # g off: both element-wise
         [(0, 0, k, 0) for k in (1, 2, 3)] +                    # exp_avg a view at an odd offset
         [(0, 0, 0, k) for k in (1, 2, 3)] +                    # exp_avg_sq likewise
         [(1, 1, 1, 1), (3, 2, 1, 0)])                          # a whole parameter set inside a flat buffer
ALIGN_CLIP_ONLY = [0, 1, 2, 3]                                  # the clip-only loop, aligned and off


@pytest.mark.parametrize("side", sorted(OM.SIDES))
@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 1023, 1025, 16383, 16384, 16385, 32769])
def test_every_alignment_at_every_chunk_edge(n, side):
    """n around the f32x4 width (tail loop only, no tail, one tail element), the 256 threads x 4 sweep, and one, two and
    three 16 K chunks with a one-element last chunk; Adam step 2, so that both moments enter."""
    hp = OM.HYPER["defaults"]
    rig = Rig([n] * len(ALIGN), [n] * len(ALIGN_CLIP_ONLY), ALIGN + ALIGN_CLIP_ONLY, hp=hp)
    assert rig.paths() == (11, 8, 1, 14, 4)
    before = OM.make_inputs(rig.sizes, rig.clip_only, seed=n, step=2, norm=OM.SIDES[side] * hp["max_norm"], max_norm=hp["max_norm"])
    rig.load(before, 2)
    rig.step(f"align n={n} {side}", before)


# ---------------------------------------------------------------------------------------------------------------------
# b. hyper-parameters
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", sorted(OM.SIDES))
@pytest.mark.parametrize("step", OM.STEPS)
@pytest.mark.parametrize("row", sorted(OM.HYPER))
def test_hyper_parameters_early_and_late(row, step, side):
    """The rows and inputs on which tests/test_optim_model.py shows the comparison to reject wrong updates; one tensor
    takes the element-wise form."""
    hp = OM.HYPER[row]
    rig = Rig(OM.HYPER_SIZES, OM.HYPER_CLIP_ONLY, [(0, 0, 0, 0), (0, 0, 0, 0), (2, 2, 2, 2), 1], hp=hp)
    seed = 1000 * sorted(OM.HYPER).index(row) + 10 * OM.STEPS.index(step) + sorted(OM.SIDES).index(side)
    before = OM.make_inputs(OM.HYPER_SIZES, OM.HYPER_CLIP_ONLY, seed=seed, step=step,
                            norm=OM.SIDES[side] * (hp["max_norm"] or 1.0), max_norm=hp["max_norm"])
    rig.load(before, step)
    _, after, _ = rig.step(f"hyper {row} t={step} {side}", before)
    assert int(rig.opt.state[rig.params[0]]["step"]) == step
    if hp["lr"] == 0.0:                                         # nothing moves but the moments
        for pb, pa, mb, ma in zip(before["p"][:3], after["p"], before["m"], after["m"]):
            assert np.array_equal(pb.view(np.uint32), pa.view(np.uint32)) and not np.array_equal(mb, ma)
    if not hp["max_norm"]:                                      # no clipping: the norm is reported all the same
        n64 = OM.grad_norm64(before["g"])
        assert abs(float(rig.opt.last_grad_norm) - n64) <= OM.NORM_TOL * n64 and n64 > 0.2


# ---------------------------------------------------------------------------------------------------------------------
# c. tensor tables (80 tensors per launch)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", sorted(OM.SIDES))
@pytest.mark.parametrize("total", [1, 2, 80, 81, 82, 160, 161, 162])
def test_tensor_table_boundaries_share_one_norm(total, side):
    """`total` tensors in all: small ones of 37..200 elements, every ninth clip-only, and (from 2 on) one of 16385
    elements, placed last among the optimised ones.  1, 80, 160: full tables and no more; 81, 161: a table of one;
    82, 162: that table holds the two-chunk tensor.  Every tensor is compared under the one reported norm."""
    small = [37 + (i * 53) % 164 for i in range(total - 1 if total > 1 else 1)]
    lazy = small[8::9]
    own = [n for i, n in enumerate(small) if i % 9 != 8] + ([16385] if total > 1 else [])
    assert len(own) + len(lazy) == total and min(small) >= 37 and max(small) <= 200
    hp = OM.HYPER["defaults"]
    offs = [((i % 4,) * 4 if i % 5 == 4 else (0, 0, 0, 0)) for i in range(len(own))] + [i % 4 for i in range(len(lazy))]
    rig = Rig(own, lazy, offs, hp=hp)
    before = OM.make_inputs(own, lazy, seed=total, step=2, norm=OM.SIDES[side] * hp["max_norm"], max_norm=hp["max_norm"])
    rig.load(before, 2)
    rig.step(f"tables total={total} {side}", before)


# ---------------------------------------------------------------------------------------------------------------------
# d. the capturable form, eager
# ---------------------------------------------------------------------------------------------------------------------
def _fresh_grads(rig, seed, norm):
    g = OM.make_inputs(rig.sizes, rig.clip_only, seed=seed, step=1, norm=norm, max_norm=rig.hp["max_norm"])["g"]
    rig.flat["g"].write(g)


def test_capturable_steps_alternate_unclipped_and_clipped():
    """Four steps of the capturable form, norm 0.25, 4, 0.25, 4 x max_norm, each compared with the model at the step
    the device counter held, from the values the previous step left."""
    hp = OM.HYPER["defaults"]
    rig = Rig([1023, 16385, 5], [255], [(0, 0, 0, 0), (0, 0, 0, 0), (1, 1, 1, 1), 0], hp=hp, capturable=True)
    rig.load(OM.make_inputs(rig.sizes, rig.clip_only, seed=40, step=1, norm=0.25, max_norm=1.0), 1)
    for k in range(4):
        side = "clipped" if k % 2 else "unclipped"
        _fresh_grads(rig, 41 + k, OM.SIDES[side] * hp["max_norm"])
        rig.step(f"capturable eager t={k + 1} {side}")
        assert rig.counters().tolist() == [k + 1.0] * 3


@pytest.mark.parametrize("count", [255, 256, 257, 513])
def test_step_counters_advance_in_groups_of_256(count):
    """255: one partial group; 256: exactly one group and no trailing launch; 257 and 513: the flush inside the loop,
    then a group of one.  Every counter advances by exactly 1.0 per step (Rig.step), parameters match at steps 1, 2, 3."""
    hp = OM.HYPER["defaults"]
    sizes = [4 + (i * 7) % 37 for i in range(count)]
    rig = Rig(sizes, [9], hp=hp, capturable=True)
    rig.load(OM.make_inputs(sizes, [9], seed=count, step=1, norm=4.0, max_norm=1.0), 1)
    for k in range(3):
        _fresh_grads(rig, count + k, (4.0, 0.25, 4.0)[k])
        rig.step(f"counters count={count} t={k + 1}")
        c = rig.counters()
        assert c.shape == (count,) and (c == k + 1.0).all()


def test_tensor_lr_filled_between_steps_takes_effect_on_the_next():
    hp = OM.HYPER["defaults"]
    rig = Rig([1023, 5], hp=hp, capturable=True, lr_tensor=True)
    rig.load(OM.make_inputs(rig.sizes, [], seed=50, step=1, norm=4.0, max_norm=1.0), 1)
    rig.step("tensor lr t=1", hp=dict(hp, lr=float(np.float32(1e-3))))
    rig.lr.fill_(2.5e-4)
    _fresh_grads(rig, 51, 0.25)
    before, after, _ = rig.step("tensor lr t=2", hp=dict(hp, lr=float(np.float32(2.5e-4))))
    with pytest.raises(AssertionError):                         # and the old lr does not describe that step
        OM.compare_step(before, after, np.float32(rig.opt.last_grad_norm.item()), step=2, **dict(hp, lr=1e-3))


def test_capturable_clip_only_launch_moves_no_parameter_and_no_counter():
    """No optimised parameter has a gradient this step, the norm_params do: the launch without a step counter."""
    hp = OM.HYPER["defaults"]
    rig = Rig([1023, 5], [255, 16385], [(0, 0, 0, 0), (0, 0, 0, 0), 1, 0], hp=hp, capturable=True)
    before = OM.make_inputs(rig.sizes, rig.clip_only, seed=60, step=3, norm=4.0, max_norm=1.0)
    rig.load(before, 3)
    for q in rig.params:
        q.grad = None
    rig.opt.step()
    torch.cuda.synchronize()
    after = rig.snapshot()
    assert rig.counters().tolist() == [2.0, 2.0]
    for r in "pmv":
        for b, a in zip(before[r][:2], after[r][:2]):
            assert np.array_equal(b.view(np.uint32), a.view(np.uint32)), r
    for b, a in zip(before["g"][:2], after["g"][:2]):           # not part of the step: neither in the norm nor scaled
        assert np.array_equal(b.view(np.uint32), a.view(np.uint32))
    lazy = dict(p=[None, None], g=before["g"][2:], m=[None, None], v=[None, None])
    worst = OM.compare_step(lazy, dict(lazy, g=after["g"][2:]), np.float32(rig.opt.last_grad_norm.item()), step=3, **hp)
    _report("capturable clip-only launch", worst)


@pytest.mark.parametrize("step", OM.STEPS)
def test_capturable_and_host_step_forms_agree_bit_for_bit(step):
    """Both form bc1 and sqrt(bc2) in double from the same step and round once; everything else is the same kernel."""
    hp = OM.HYPER["defaults"]
    out = []
    for capturable in (False, True):
        rig = Rig(OM.HYPER_SIZES, OM.HYPER_CLIP_ONLY, [(0, 0, 0, 0), (0, 0, 0, 0), (2, 2, 2, 2), 1], hp=hp, capturable=capturable)
        before = OM.make_inputs(OM.HYPER_SIZES, OM.HYPER_CLIP_ONLY, seed=70 + step, step=step, norm=4.0, max_norm=1.0)
        rig.load(before, step)
        _, after, _ = rig.step(f"forms agree t={step} capturable={capturable}", before, report=False)
        out.append((after, rig.opt.last_grad_norm.item()))
    (a, na), (b, nb) = out
    assert na == nb
    for r in "pgmv":
        for x, y in zip(a[r], b[r]):
            assert (x is None and y is None) or np.array_equal(x.view(np.uint32), y.view(np.uint32)), r


# ---------------------------------------------------------------------------------------------------------------------
# e. non-finite and degenerate values
# ---------------------------------------------------------------------------------------------------------------------
# Every finite gradient here is at most a few units, and the largest case has 20 K elements: every square and every
# sum of squares stays far inside fp32 range.  An fp32 overflow of the square sum is torch's behaviour too and is not
# under test.
def test_one_infinite_gradient_element():
    """norm inf, coef 0: that element NaN (inf * 0), every other gradient 0; the parameters move by weight decay alone
    and are NaN only where the model (and torch) put it."""
    hp = OM.HYPER["moved"]                                      # weight decay 0.1: large enough to be seen moving
    rig = Rig([1023, 16385, 5], [255], hp=hp)
    before = OM.make_inputs(rig.sizes, rig.clip_only, seed=80, step=2, norm=2.0, max_norm=hp["max_norm"])
    before["g"][1][16384] = np.float32(math.inf)                # the lone element of the second chunk
    rig.load(before, 2)
    _, after, _ = rig.step("one +inf gradient", before)
    assert math.isinf(rig.opt.last_grad_norm.item())
    assert np.isnan(after["g"][1][16384]) and np.isnan(after["p"][1][16384])
    assert sum(int(np.isnan(a).sum()) for a in after["p"][:3]) == 1 == sum(int(np.isnan(a).sum()) for a in after["g"])
    assert all((np.nan_to_num(a, nan=0.0) == 0).all() for a in after["g"])
    assert all(not np.array_equal(b, a) for b, a in zip(before["p"][:3], after["p"][:3]))


def test_one_nan_gradient_poisons_both_tensor_tables():
    hp = OM.HYPER["defaults"]
    sizes = [37 + i for i in range(100)]
    rig = Rig(sizes, [50], hp=hp)
    before = OM.make_inputs(sizes, [50], seed=81, step=2, norm=0.25, max_norm=1.0)
    before["g"][90][3] = np.float32("nan")                      # a tensor of the second table
    rig.load(before, 2)
    _, after, _ = rig.step("one NaN gradient, two tables", before)
    assert math.isnan(rig.opt.last_grad_norm.item())
    for r in "pgmv":
        assert all(a is None or np.isnan(a).all() for a in after[r]), r


def test_zero_gradients_without_weight_decay_change_nothing():
    hp = OM.HYPER["nowd_noclip"]
    for max_norm in (None, 1.0):
        hp = dict(hp, max_norm=max_norm)
        rig = Rig([1023, 16385, 5], [255], [(0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 0, 0), 0], hp=hp)
        before = OM.make_inputs(rig.sizes, rig.clip_only, seed=82, step=1, norm=1.0, max_norm=max_norm)
        before["g"] = [np.zeros_like(g) for g in before["g"]]
        rig.load(before, 1)
        _, after, _ = rig.step(f"zero gradients max_norm={max_norm}", before)
        assert rig.opt.last_grad_norm.item() == 0.0
        for r in "pgmv":
            for b, a in zip(before[r], after[r]):
                assert (b is None and a is None) or np.array_equal(b.view(np.uint32), a.view(np.uint32)), r


def test_gradients_whose_squares_are_subnormal():
    """Gradients of about 1e-22: k * 2^-74 with |k| <= 3 (2^-73 = 1.06e-22), so that every square k^2 * 2^-148 is an
    fp32 subnormal that is exact, the sum of squares is exact too, and the 1e-5 bound on the norm means what it says
    (a kernel that flushed subnormals would report 0).  Weight decay keeps the update itself in the normal range."""
    hp = OM.HYPER["defaults"]
    rig = Rig([1023, 16385, 5], [255], [(0, 0, 0, 0), (0, 0, 0, 0), (3, 3, 3, 3), 2], hp=hp)
    before = OM.make_inputs(rig.sizes, rig.clip_only, seed=83, step=2, norm=0.25, max_norm=1.0)
    rng = np.random.RandomState(83)
    before["g"] = [(rng.randint(-3, 4, size=g.shape) * 2.0 ** -74).astype(np.float32) for g in before["g"]]
    assert all(((g.astype(np.float64) ** 2) < 2.0 ** -126).all() for g in before["g"])
    rig.load(before, 2)
    rig.step("subnormal squares", before)
    n64 = OM.grad_norm64(before["g"])
    assert 1e-21 < n64 < 1e-19 and abs(rig.opt.last_grad_norm.item() - n64) <= OM.NORM_TOL * n64


# ---------------------------------------------------------------------------------------------------------------------
# f. captured replays of the unclipped / clipped alternation
# ---------------------------------------------------------------------------------------------------------------------
def test_three_captured_replays_equal_three_eager_steps():
    """The capture pattern of tests/test_graph_step_gpu.py part 3 with gradients that start BELOW the clip threshold:
    warm-up step on a side stream, capture of (load gradients, step), then replays at norm 0.25, 4, 0.25 x max_norm
    against the same steps run eagerly: parameters, gradients, moments, counters and the reported norm bit-equal."""
    from wf3d.optim import ClipAdam
    hp = OM.HYPER["defaults"]
    sizes = [1023, 16385, 5, 200]
    ins = OM.make_inputs(sizes, [], seed=90, step=1, norm=0.25, max_norm=1.0)
    g0 = [torch.from_numpy(g).to(dev()) for g in ins["g"]]

    def make():
        ps = [torch.nn.Parameter(torch.from_numpy(p).to(dev())) for p in ins["p"][:4]]
        for p in ps:
            p.grad = torch.zeros_like(p)
        return ps, ClipAdam(ps, lr=hp["lr"], weight_decay=hp["weight_decay"], max_norm=hp["max_norm"], capturable=True)

    (pg, og), (pe, oe) = make(), make()
    scale = torch.ones((), device=dev())

    def load_and_step(ps, opt):
        for p, g in zip(ps, g0):
            p.grad.copy_(g * scale)
        opt.step()

    s = torch.cuda.Stream(dev())
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        load_and_step(pg, og)                                   # warm-up: creates the state
    torch.cuda.current_stream().wait_stream(s)
    load_and_step(pe, oe)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        load_and_step(pg, og)
    norms = []
    for k, sc in enumerate((1.0, 16.0, 1.0)):
        scale.fill_(sc)
        graph.replay()
        norms.append(og.last_grad_norm.clone())
        load_and_step(pe, oe)
        assert torch.equal(norms[-1], oe.last_grad_norm)
    torch.cuda.synchronize()
    assert [round(float(n), 3) for n in norms] == [0.25, 4.0, 0.25]
    for a, b in zip(pg, pe):
        assert torch.equal(a, b) and torch.equal(a.grad, b.grad)
        for key in ("exp_avg", "exp_avg_sq", "step"):
            assert torch.equal(og.state[a][key], oe.state[b][key]), key
        assert float(og.state[a]["step"]) == 4.0


def test_zz_report_the_largest_errors_of_this_file():
    """Prints the maxima over the cases above (they run first in file order); asserts nothing new."""
    for k, (v, label) in sorted(WORST.items()):
        print(f"[optim forms] LARGEST {k}: {v:.3e}  ({label})")
    assert all(v <= (1.0 if k == "dp_bound" else OM.NORM_TOL if k == "norm" else OM.TOL) for k, (v, _) in WORST.items())
