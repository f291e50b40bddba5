"""Row f-2: the tail of the reference's training step (train.py:141-142),

    torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=1.0)
    optimizer.step()                                   # Adam(lr=1e-3, weight_decay=1e-6), train.py:96

as two kernel launches over all parameter tensors (csrc/optim.hip) instead of ~500 small foreach kernels.

    opt = ClipAdam(model.parameters(), lr=1e-3, weight_decay=1e-6, max_norm=1.0, norm_params=model.parameters)
    ...
    loss.backward()
    opt.step()              # clip (in place, over norm_params) + Adam (over the optimizer's own parameters)

`norm_params` is a callable so that parameters created AFTER the optimizer — the reference's lazy
`vertex_predictor.point_pool_proj`, SURVEY.md §9 Q1 — enter the global norm and get their gradient scaled exactly as
`clip_grad_norm_(model.parameters())` does, while never being updated (they are not in the optimizer, as in train.py).
State (`step`, `exp_avg`, `exp_avg_sq`) uses torch.optim.Adam's names, so `state_dict()` round-trips with it.

capturable=True (torch.optim.Adam(capturable=True)'s layout and meaning): `state["step"]` is a 0-d fp32 tensor on the
parameter's device, read by the kernel and advanced on the device (wf3d_clip_adam_step_dev), and `lr` may be a 0-d
device tensor (a scheduler `fill_`s it), so `opt.step()` can be captured into a CUDA graph and replayed: each replay
applies the next step's bias corrections and the current lr.  The state must exist before the capture (a warm-up step
creates it).  A non-capturable ClipAdam refuses to step inside a capture: its step counter and lr are host values that
a graph would freeze.

Parameter groups (up to 16) take torch's keys `lr`, `betas`, `eps`, `weight_decay` and `decoupled_weight_decay`
(torch.optim.AdamW's decay: the parameter loses lr * weight_decay * p, the gradient enters the moments as it is);
`max_norm`, `norm_params`, `capturable` and `skip_nonfinite` belong to the optimizer: there is ONE global norm and one
clip coefficient over every tensor of every group, as `clip_grad_norm_(model.parameters())` has.  `add_param_group`
works before and after steps; a group that joins later starts at Adam step 1 beside groups that are further on.  On the
host form every tensor of one group must be at one step (groups may differ); the capturable form keeps a device counter
per tensor, so there any tensor may be at any step.

    opt = ClipAdam([{"params": encoder, "lr": 1e-4}, {"params": gains_and_biases, "weight_decay": 0.0}, {"params": rest}],
                   lr=1e-3, weight_decay=1e-2, decoupled_weight_decay=True, max_norm=1.0, norm_params=model.parameters)

skip_nonfinite=True (capturable only): a step whose global gradient norm is NaN or infinite writes no gradient, parameter,
moment or step counter; `opt.skipped_steps` (a device int64 scalar, created by the first step and never read by step())
counts such steps and `last_grad_norm` still holds the norm.  The decision is taken on the device, so it also holds
in a replayed graph where nothing on the host sees the gradient.  The norm's sum of squares is an fp32 sum: finite
gradients of norm above 1.8e19 overflow it and count as non-finite.  Without the flag a NaN poisons every tensor, as
clip_grad_norm_ does.

One group without decoupled decay and without the skip, all of whose tensors are at one step, runs the single-group
kernels (wf3d_clip_adam_step / _dev); everything else runs wf3d_clip_adam_step_groups, with the tensors in
`norm_params`' order where it is given: the norm's partial sums are folded in table order, so the same tensors spread
over groups in any way give the norm — and, with equal hyper-parameters, the step — of one group, bit for bit.

Learning-rate schedules (`lr_schedule`, a constructor default and a group key like `lr`; None: no schedule) are plain
dicts, and `lr_factor(schedule, t)` below is their specification: warm-up times decay, as a function of the number t
of updates this optimizer has applied.  `group["lr"]` stays the base rate; the rate applied is float32(lr * factor).

    opt = ClipAdam(params, lr=1e-3, capturable=True, skip_nonfinite=True,
                   lr_schedule=dict(warmup_steps=500, warmup_start=0.01, decay="cosine", decay_steps=20000, min_factor=0.01))

`opt.schedule_step` is that t, one per optimizer as a torch scheduler has one `last_epoch`.  While some group has a
schedule it grows by one in every step that advances at least one Adam counter: not in a skipped step, not in a step
of clip-only tensors alone (without any schedule nothing reads it, and it stays where it is in both forms).
`set_schedule_step(t)` places it (before a capture); `state_dict()` carries it as the top-level key "schedule_step",
which torch.optim.Adam ignores, and a dict without it leaves the count at 0.  Host form: a Python int, `lr_factor` is
evaluated on the host and `last_lr` is a CPU fp32 tensor.  Capturable form: a 0-d int64 device tensor that the first
scheduled step creates (like `skipped_steps`; a step inside a capture before that raises), read by one small launch
(lr_schedule_kernel, one thread per group) that writes the rates into `opt.last_lr`, an fp32 device tensor with one
entry per group, where the Adam launches read them: `last_lr` is what was applied, not a second computation of it.
The count advances on the device, under the skip's own decision, so a captured step needs no `fill_` between replays
and a warm-up keyed to "updates applied" stays right when steps are skipped.  A group without a schedule gets its
base rate in `last_lr`; a group whose `lr` is itself a device tensor gets no write and its entry stays NaN (a
schedule beside a tensor `lr` in one group is refused).  `last_lr` exists only while some group has a schedule.

Averaged weights (`ema_decay`, a constructor default and a group key; None or 0: that group keeps no average;
`ema_warmup` belongs to the optimizer): `state[p]["ema"]`, fp32 of the parameter's shape, is created with the rest of
the state as a copy of the parameter before its first update, travels in the state dict, and follows every applied
update in the pass that stores the new parameter value p':  ema' = fmaf(1 - d, p' - ema, ema), with 1 - d rounded once
from double and, under `ema_warmup`, d = min(ema_decay, (1 + n) / (10 + n)) for the tensor's Adam step n before the
update.  A skipped step leaves the average alone; lr = 0 still moves it towards the unchanged parameter.  p, g, m, v
and the norm are bit for bit those of the step without the average.  `swap_ema()` exchanges parameters and averages
(capturable; twice is the identity, bit for bit), `with opt.ema_weights():` swaps in and back out, and `step()` while
swapped raises (a swap replayed from a graph is invisible to the host: that check follows eager swaps only).  Every rank of a data-parallel run holds the same averages because it holds the same parameters:
nothing is reduced.

Any group with an average, and in the capturable form any group with a schedule, takes wf3d_clip_adam_step_ema;
everything else takes the routes above, with the kernels and the bits it had before these options existed."""
import contextlib
import ctypes
import math

import torch

from . import _lib
from ._lib import check
from .ops import _stream

MAX_GROUPS = 16     # the kernel-argument table of wf3d_clip_adam_step_groups
MAX_MILESTONES = 8  # of a multistep decay: wf3d_lr_schedule's table
DECAYS = ("constant", "cosine", "linear", "exponential", "multistep")     # at the index of its WF3D_LR_* value
_NO_SCHEDULE = dict(warmup_steps=0, warmup_start=0.0, decay="constant", decay_steps=0, min_factor=0.0, gamma=1.0, milestones=())


def check_schedule(schedule):
    """The schedule with every key present (a copy), or ValueError.  Keys: warmup_steps (0), warmup_start (0.0),
    decay ("constant"; one of DECAYS), decay_steps (cosine and linear need it, >= 1), min_factor (0.0), gamma
    (exponential and multistep need it, in (0, 1]), milestones (multistep: at most 8, non-decreasing, repeats allowed)."""
    if not isinstance(schedule, dict):
        raise ValueError(f"ClipAdam: lr_schedule must be a dict or None, got {type(schedule).__name__}")
    unknown = set(schedule) - set(_NO_SCHEDULE)
    if unknown:
        raise ValueError(f"ClipAdam: unknown lr_schedule keys {sorted(unknown)} (known: {sorted(_NO_SCHEDULE)})")
    s = dict(_NO_SCHEDULE, **schedule)
    kind = s["decay"]
    if kind not in DECAYS:
        raise ValueError(f"ClipAdam: unknown lr_schedule decay {kind!r} (known: {DECAYS})")
    for key in ("warmup_steps", "decay_steps"):
        if isinstance(s[key], bool) or int(s[key]) != s[key]:
            raise ValueError(f"ClipAdam: lr_schedule {key} must be an integer, got {s[key]!r}")
        s[key] = int(s[key])
    if s["warmup_steps"] < 0:
        raise ValueError("ClipAdam: lr_schedule warmup_steps must be >= 0")
    if kind in ("cosine", "linear") and s["decay_steps"] < 1:
        raise ValueError(f"ClipAdam: lr_schedule decay={kind!r} needs decay_steps >= 1")
    for key in ("warmup_start", "min_factor"):
        s[key] = float(s[key])
        if not 0.0 <= s[key] <= 1.0:
            raise ValueError(f"ClipAdam: lr_schedule {key} must be in [0, 1], got {s[key]}")
    if kind in ("exponential", "multistep") and "gamma" not in schedule:
        raise ValueError(f"ClipAdam: lr_schedule decay={kind!r} needs gamma")
    s["gamma"] = float(s["gamma"])
    if not 0.0 < s["gamma"] <= 1.0:
        raise ValueError(f"ClipAdam: lr_schedule gamma must be in (0, 1], got {s['gamma']}")
    ms = tuple(int(m) for m in s["milestones"])
    if len(ms) > MAX_MILESTONES:
        raise ValueError(f"ClipAdam: lr_schedule has {len(ms)} milestones (at most {MAX_MILESTONES})")
    if any(b < a for a, b in zip((0,) + ms, ms)):
        raise ValueError(f"ClipAdam: lr_schedule milestones must be non-negative and non-decreasing, got {ms}")
    s["milestones"] = ms
    return s


def lr_factor(schedule, t):
    """The factor on the base rate of the update that follows `t` applied updates (t = 0: the first), in float64: the
    text that lr_schedule_kernel is held to, operation for operation.  None or {}: exactly 1.0.

        fw = warmup_start + (1 - warmup_start) t / warmup_steps     for t < warmup_steps, else 1
        u = max(t - warmup_steps, 0),  T = decay_steps
        fd = 1                                                               "constant"
             min_factor + (1 - min_factor) (1 + cos(pi min(u, T) / T)) / 2   "cosine"
             1 + (min_factor - 1) min(u, T) / T                              "linear"
             max(gamma ** u, min_factor)                                     "exponential"
             gamma ** (number of milestones <= u)                            "multistep"
        factor = fw fd

    It is torch's LinearLR followed by CosineAnnealingLR / LinearLR / ExponentialLR / MultiStepLR under
    SequentialLR(milestones=[warmup_steps]), up to and including the end of the decay.  Past T, cosine and linear STAY at
    min_factor; torch's CosineAnnealingLR turns back up there.  Schedules that restart are not offered."""
    s = check_schedule(schedule or {})
    t = int(t)
    W, T, ws, mf, gamma = s["warmup_steps"], s["decay_steps"], s["warmup_start"], s["min_factor"], s["gamma"]
    fw = ws + (1.0 - ws) * t / W if t < W else 1.0
    u = max(t - W, 0)
    kind = s["decay"]
    if kind == "cosine":
        fd = mf + (1.0 - mf) * 0.5 * (1.0 + math.cos(math.pi * min(u, T) / T))
    elif kind == "linear":
        fd = 1.0 + (mf - 1.0) * min(u, T) / T
    elif kind == "exponential":
        fd = max(gamma ** float(u), mf)
    elif kind == "multistep":
        fd = gamma ** float(sum(m <= u for m in s["milestones"]))
    else:
        fd = 1.0
    return fw * fd


class ClipAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_norm=None, norm_params=None,
                 capturable=False, decoupled_weight_decay=False, skip_nonfinite=False, lr_schedule=None, ema_decay=None,
                 ema_warmup=False):
        for name, flag in (("capturable", capturable), ("skip_nonfinite", skip_nonfinite), ("ema_warmup", ema_warmup)):
            if not isinstance(flag, bool):
                raise TypeError(f"ClipAdam: {name} must be a bool, got {type(flag).__name__}")
        if skip_nonfinite and not capturable:
            raise ValueError("ClipAdam: skip_nonfinite=True needs capturable=True (the non-capturable step advances its step "
                             "counters on the host, which cannot know that the device skipped)")
        self.capturable = capturable        # add_param_group (called by the base constructor) reads it
        # read by step() and by set_schedule_step(); the capturable form's count is None until a scheduled step creates it
        self.schedule_step = None if capturable else 0
        self._schedule_start = 0            # capturable: where the first scheduled step starts the device count
        self.last_lr = None                 # fp32 [groups]: the rates of the last step, while some group has a schedule
        self.ema_warmup = ema_warmup
        self._ema_swapped = False
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                                      decoupled_weight_decay=decoupled_weight_decay, capturable=capturable,
                                      lr_schedule=lr_schedule, ema_decay=ema_decay))
        self.max_norm = max_norm
        self.skip_nonfinite = skip_nonfinite
        self._norm_params = norm_params
        self.last_grad_norm = None          # device scalar: pre-clip global L2 norm of the last step
        self.skipped_steps = None           # device int64 scalar (skip_nonfinite): steps skipped so far
        # capturable: do all step counters move together, as far as the host can tell without reading one?  Cleared for
        # good by a step in which a tensor joins or sits out; such an optimizer steps by per-tensor counters from then on
        self._lockstep = True

    def _check_group(self, group):
        lr, betas = group["lr"], group["betas"]
        if torch.is_tensor(lr):
            if not self.capturable:
                raise ValueError("ClipAdam: a tensor lr needs capturable=True (a non-capturable step reads lr on the host)")
            if lr.numel() != 1 or lr.dim() != 0 or lr.dtype != torch.float32:
                raise ValueError("ClipAdam: a tensor lr must be a 0-d fp32 tensor")
            if float(lr) < 0:
                raise ValueError("ClipAdam: bad hyper-parameters")
        elif lr < 0:
            raise ValueError("ClipAdam: bad hyper-parameters")
        if group["eps"] < 0 or not (0 <= betas[0] < 1 and 0 <= betas[1] < 1) or group["weight_decay"] < 0:
            raise ValueError("ClipAdam: bad hyper-parameters")
        if not isinstance(group["decoupled_weight_decay"], bool):
            raise TypeError("ClipAdam: decoupled_weight_decay must be a bool")
        if group["lr_schedule"] is not None:
            if torch.is_tensor(lr):
                raise ValueError("ClipAdam: a group takes a tensor lr or an lr_schedule, not both (the schedule writes the "
                                 "rate it applies into last_lr)")
            group["lr_schedule"] = check_schedule(group["lr_schedule"])
        d = group["ema_decay"]
        if d is not None and not (isinstance(d, (int, float)) and not isinstance(d, bool) and 0 <= d < 1):
            raise ValueError(f"ClipAdam: ema_decay must be None or a number in [0, 1), got {d!r}")

    def add_param_group(self, param_group):
        if len(self.param_groups) >= MAX_GROUPS:
            raise ValueError(f"ClipAdam: at most {MAX_GROUPS} parameter groups (the group table travels as kernel arguments)")
        super().add_param_group(param_group)
        group = self.param_groups[-1]
        try:
            self._check_group(group)
        except (TypeError, ValueError):
            self.param_groups.pop()
            raise
        group["capturable"] = self.capturable

    def load_state_dict(self, state_dict):
        # the saved groups' "capturable" (torch.optim.Adam writes one) does not change how this optimizer steps; step
        # counters of the other layout are converted at the next step()
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            group["capturable"] = self.capturable
            for key in ("decoupled_weight_decay", "lr_schedule", "ema_decay"):
                group.setdefault(key, self.defaults[key])
            self._check_group(group)
        # the one place where the host may look at the loaded counters
        self._lockstep = len({float(st["step"]) for st in self.state.values() if "step" in st}) <= 1
        self.set_schedule_step(int(state_dict.get("schedule_step", 0)))
        self._ema_swapped = bool(state_dict.get("ema_swapped", False))

    def state_dict(self):
        """torch's layout, plus two top-level keys that torch.optim.Adam's load_state_dict does not read:
        "schedule_step" (an int; the capturable form reads its device count here) and "ema_swapped"."""
        sd = super().state_dict()
        t = self.schedule_step
        sd["schedule_step"] = self._schedule_start if t is None else int(t)
        sd["ema_swapped"] = self._ema_swapped
        return sd

    def set_schedule_step(self, t):
        """Place the schedules' count of applied updates; in the capturable form before the capture."""
        if isinstance(t, bool) or int(t) != t or t < 0:
            raise ValueError(f"ClipAdam: schedule_step must be a non-negative integer, got {t!r}")
        if not self.capturable:
            self.schedule_step = int(t)
        elif self.schedule_step is None:
            self._schedule_start = int(t)
        else:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("ClipAdam: set_schedule_step() inside a capture would freeze the value into the graph")
            self.schedule_step.fill_(int(t))

    def _averaged(self):
        """(parameter, average) of every tensor that has one."""
        return [(p, self.state[p]["ema"]) for group in self.param_groups for p in group["params"]
                if p in self.state and "ema" in self.state[p]]

    @torch.no_grad()
    def swap_ema(self):
        """Parameters and averages change places (wf3d_ema_swap; capturable).  Tensors without an average are untouched."""
        pairs = self._averaged()
        if not pairs:
            raise RuntimeError("ClipAdam: swap_ema() before any parameter has an average (ema_decay, and one step)")
        for p, e in pairs:
            if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and e.is_cuda and e.dtype == torch.float32
                    and e.is_contiguous() and e.numel() == p.numel()):
                raise RuntimeError("ClipAdam: swap_ema() needs contiguous fp32 CUDA parameters and averages of their size")
        n = len(pairs)
        vp = ctypes.c_void_p * n
        check(_lib.load().wf3d_ema_swap(vp(*[p.data_ptr() for p, _ in pairs]), vp(*[e.data_ptr() for _, e in pairs]),
                                        (ctypes.c_long * n)(*[p.numel() for p, _ in pairs]), n, _stream()), "ema_swap")
        for p, _ in pairs:
            torch.autograd.graph.increment_version(p)
        # a swap recorded into a graph moves nothing now and anything later: the flag follows eager swaps only
        if not torch.cuda.is_current_stream_capturing():
            self._ema_swapped = not self._ema_swapped

    @contextlib.contextmanager
    def ema_weights(self):
        """`with opt.ema_weights():` — the model holds the averaged weights inside the block."""
        self.swap_ema()
        try:
            yield self
        finally:
            self.swap_ema()

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        groups = self.param_groups
        capturable = self.capturable
        capturing = torch.cuda.is_current_stream_capturing()
        if not capturable and capturing:
            raise RuntimeError("ClipAdam: step() inside a CUDA graph capture needs ClipAdam(..., capturable=True): the "
                               "non-capturable step reads its step counter and lr on the host, which a graph would freeze")
        if self._ema_swapped:
            raise RuntimeError("ClipAdam: step() while the averaged weights are swapped in (swap_ema() again first)")
        by_group = [[p for p in group["params"] if p.grad is not None] for group in groups]
        own = by_group[0] if len(groups) == 1 else [p for ps in by_group for p in ps]
        own_ids = {id(p) for group in groups for p in group["params"]}
        extra, src = [], []
        if self._norm_params is not None:
            src = list(self._norm_params() if callable(self._norm_params) else self._norm_params)
            extra = [p for p in src if id(p) not in own_ids and p.grad is not None]       # a group's tensor counts once
        if not own and not extra:
            return loss
        # validate everything and collect the pointers FIRST; the per-parameter step counters are advanced only after the
        # launch has been accepted, so that a failed step leaves the optimizer where it was and can simply be retried
        gsteps = [set() for _ in groups]            # host form: the 1-based step of each group's tensors
        fresh = set()                               # capturable: is there state?  (no device step is read here)
        for ps, steps in zip(by_group, gsteps):
            for p in ps:
                g = p.grad
                if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and g.is_cuda and g.dtype == torch.float32):
                    raise RuntimeError("ClipAdam: contiguous fp32 CUDA parameters (and fp32 CUDA gradients) only")
                st = self.state[p]
                if capturable:
                    fresh.add(not st)
                    if capturing and not st:
                        raise RuntimeError("ClipAdam(capturable=True): run one step before the capture (it creates the state)")
                else:
                    steps.add(int(st["step"]) + 1 if st else 1)
        for p in extra:
            g = p.grad
            if not (g.is_cuda and g.dtype == torch.float32):
                raise RuntimeError("ClipAdam: the clip-only tensors of norm_params need fp32 CUDA gradients "
                                   f"(got {g.dtype} on {g.device})")
        for k, s in enumerate(gsteps):
            if len(s) > 1:
                raise RuntimeError(f"ClipAdam: the parameters of group {k} are at different Adam steps {sorted(s)} (a parameter "
                                   "without gradient in an earlier step); put them into groups of their own, or use "
                                   "capturable=True, which keeps a step counter per tensor")
        for group in groups:
            lr = group["lr"]
            if torch.is_tensor(lr) and not (capturable and lr.is_cuda and lr.dtype == torch.float32 and lr.dim() == 0):
                raise RuntimeError("ClipAdam: a tensor lr must be a 0-d fp32 CUDA tensor, with capturable=True")
        dev = (own or extra)[0].device
        if self.skip_nonfinite and self.skipped_steps is None:
            if capturing:
                raise RuntimeError("ClipAdam(skip_nonfinite=True): run one step before the capture (it creates skipped_steps)")
            self.skipped_steps = torch.zeros((), dtype=torch.int64, device=dev)
        schedules = [group["lr_schedule"] for group in groups]
        scheduled = any(s is not None for s in schedules)
        averaged = [bool(group["ema_decay"]) for group in groups]
        dev_sched = capturable and scheduled
        if dev_sched and (self.schedule_step is None or self.last_lr is None or self.last_lr.numel() != len(groups)):
            if capturing:
                raise RuntimeError("ClipAdam(lr_schedule=...): run one step before the capture (it creates schedule_step "
                                   "and last_lr)")
            if self.schedule_step is None:
                self.schedule_step = torch.full((), self._schedule_start, dtype=torch.int64, device=dev)
            self.last_lr = torch.full((len(groups),), float("nan"), dtype=torch.float32, device=dev)
        # the new options' entry point: an average in either form, a schedule in the capturable one (the host form
        # evaluates lr_factor here and passes the product as the lr that every entry point takes)
        extended = dev_sched or any(averaged)
        host_lr = [group["lr"] if capturable or s is None else float(group["lr"]) * lr_factor(s, self.schedule_step)
                   for group, s in zip(groups, schedules)]
        if capturable:
            # a tensor that joins beside older ones, or one that has state and sits out a step the others take, leaves
            # the lockstep
            sits_out = any(p.grad is None and self.state.get(p) for group in groups for p in group["params"])
            if len(fresh) > 1 or (own and sits_out):
                self._lockstep = False
            one_step = self._lockstep
        else:
            one_step = len({t for s in gsteps for t in s}) <= 1
        single = (len(groups) == 1 and not groups[0].get("decoupled_weight_decay", False) and not self.skip_nonfinite
                  and one_step and not extended)
        K = []                                      # grouped form: each table entry's group (-1: clip-only)
        if not single:
            K = [k for k, ps in enumerate(by_group) for _ in ps]
            if src:
                # the partial sums of the norm are folded in table order: with the tensors in norm_params' order, however
                # they are spread over groups, the norm has the bits of the same tensors in one group
                rank = {id(p): i for i, p in enumerate(src)}
                order = sorted(range(len(own)), key=lambda i: rank.get(id(own[i]), len(rank)))
                own, K = [own[i] for i in order], [K[i] for i in order]
            K += [-1] * len(extra)
        S = []
        P, G, M, V, N, E = [], [], [], [], [], []
        keep = []
        for i, p in enumerate(own):
            g = p.grad
            if not g.is_contiguous():
                g = p.grad = g.contiguous()
            st = self.state[p]
            if not st:
                st["step"] = torch.zeros((), dtype=torch.float32, device=p.device) if capturable else torch.tensor(0.0)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            if extended:
                if not averaged[K[i]]:
                    E.append(None)
                else:
                    if "ema" not in st:                   # with the rest of the state, or after a state dict without one
                        if capturing:
                            raise RuntimeError("ClipAdam(ema_decay=...): the averages must exist before the capture")
                        st["ema"] = p.detach().clone(memory_format=torch.preserve_format)
                    e = st["ema"]
                    if not (e.is_cuda and e.dtype == torch.float32 and e.is_contiguous() and e.numel() == p.numel()):
                        raise RuntimeError("ClipAdam: an average must be a contiguous fp32 CUDA tensor of its parameter's size")
                    E.append(e.data_ptr())
            if capturable:
                t = st["step"]
                if not (torch.is_tensor(t) and t.device == p.device and t.dtype == torch.float32 and t.dim() == 0):
                    if capturing:
                        raise RuntimeError("ClipAdam(capturable=True): step counters must be device tensors before the capture")
                    st["step"] = torch.as_tensor(t, dtype=torch.float32).reshape(()).to(p.device).clone()
                S.append(st["step"].data_ptr())
            P.append(p.data_ptr()); G.append(g.data_ptr()); M.append(st["exp_avg"].data_ptr()); V.append(st["exp_avg_sq"].data_ptr())
            N.append(p.numel())
        for p in extra:                                   # clip-only tensors (in the norm, scaled, never updated)
            g = p.grad
            if not g.is_contiguous():
                g = p.grad = g.contiguous()
            P.append(None); G.append(g.data_ptr()); M.append(None); V.append(None); N.append(g.numel()); S.append(None)
            E.append(None)
            keep.append(g)
        n = len(G)
        vp = ctypes.c_void_p * n
        numel = (ctypes.c_long * n)(*N)
        lib = _lib.load()
        nws = lib.wf3d_clip_adam_ws_floats(numel, n)
        ws = torch.empty(nws, dtype=torch.float32, device=dev)
        norm = torch.empty((), dtype=torch.float32, device=dev)
        max_norm = float(self.max_norm or 0.0)
        if single:
            group = groups[0]
            lr = host_lr[0]
            b1, b2 = group["betas"]
            if capturable:
                # step counters and a tensor lr are read (and the counters advanced) on the device
                lr_dev = lr.data_ptr() if torch.is_tensor(lr) else None
                check(lib.wf3d_clip_adam_step_dev(vp(*P), vp(*G), vp(*M), vp(*V), vp(*S), numel, n, max_norm,
                                                  0.0 if lr_dev else float(lr), lr_dev, float(b1), float(b2), float(group["eps"]),
                                                  float(group["weight_decay"]), ws.data_ptr(), nws, norm.data_ptr(), _stream()),
                      "clip_adam_step_dev")
            else:
                step = gsteps[0].pop() if gsteps[0] else 1
                check(lib.wf3d_clip_adam_step(vp(*P), vp(*G), vp(*M), vp(*V), numel, n, max_norm, float(lr),
                                              float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]), step,
                                              ws.data_ptr(), nws, norm.data_ptr(), _stream()), "clip_adam_step")
        else:
            ng = len(groups)
            dbl, integer = ctypes.c_double * ng, ctypes.c_int * ng
            lrs = host_lr
            lr_ptr = [lr.data_ptr() if torch.is_tensor(lr) else None for lr in lrs]
            if dev_sched:
                # one thread per group writes the rate of this step into last_lr, where the Adam launches read it; a
                # group whose lr is a device tensor keeps that tensor and gets no write
                rows = [s if s is not None else _NO_SCHEDULE for s in schedules]
                lng = ctypes.c_long * ng
                ms = [m for r in rows for m in (tuple(r["milestones"]) + (0,) * MAX_MILESTONES)[:MAX_MILESTONES]]
                check(lib.wf3d_lr_schedule(
                    dbl(*[0.0 if torch.is_tensor(lr) else float(lr) for lr in lrs]), lng(*[r["warmup_steps"] for r in rows]),
                    dbl(*[r["warmup_start"] for r in rows]), integer(*[DECAYS.index(r["decay"]) for r in rows]),
                    lng(*[r["decay_steps"] for r in rows]), dbl(*[r["min_factor"] for r in rows]),
                    dbl(*[r["gamma"] for r in rows]), (ctypes.c_long * len(ms))(*ms), integer(*[len(r["milestones"]) for r in rows]),
                    integer(*[int(ptr is None) for ptr in lr_ptr]), ng, self.schedule_step.data_ptr(), self.last_lr.data_ptr(),
                    _stream()), "lr_schedule")
                lr_ptr = [self.last_lr.data_ptr() + 4 * k if ptr is None else ptr for k, ptr in enumerate(lr_ptr)]
            lr_dev = (ctypes.c_void_p * ng)(*lr_ptr)
            flags = _lib.DEFINES["WF3D_ADAM_SKIP_NONFINITE"] if self.skip_nonfinite else 0
            head = (vp(*P), vp(*G), vp(*M), vp(*V))
            tables = (numel, (ctypes.c_int * n)(*K), vp(*S) if capturable else None, n,
                      dbl(*[0.0 if torch.is_tensor(lr) else float(lr) for lr in lrs]), lr_dev,
                      dbl(*[float(group["betas"][0]) for group in groups]), dbl(*[float(group["betas"][1]) for group in groups]),
                      dbl(*[float(group["eps"]) for group in groups]), dbl(*[float(group["weight_decay"]) for group in groups]),
                      integer(*[int(group.get("decoupled_weight_decay", False)) for group in groups]))
            gstep = integer(*[next(iter(s)) if s else 1 for s in gsteps])
            skipped = self.skipped_steps.data_ptr() if self.skip_nonfinite else None
            if extended:
                if self.ema_warmup:
                    flags |= _lib.DEFINES["WF3D_ADAM_EMA_WARMUP"]
                check(lib.wf3d_clip_adam_step_ema(
                    *head, vp(*E) if any(averaged) else None, *tables, dbl(*[float(group["ema_decay"] or 0.0) for group in groups]),
                    gstep, ng, max_norm, flags, skipped, self.schedule_step.data_ptr() if dev_sched else None, ws.data_ptr(), nws,
                    norm.data_ptr(), _stream()), "clip_adam_step_ema")
            else:
                check(lib.wf3d_clip_adam_step_groups(*head, *tables, gstep, ng, max_norm, flags, skipped, ws.data_ptr(), nws,
                                                     norm.data_ptr(), _stream()), "clip_adam_step_groups")
        if not capturable:
            for p in own:
                self.state[p]["step"] += 1
            if scheduled:                                 # what was applied: the one rounding that the kernel's argument gets
                self.last_lr = torch.tensor([float(lr) for lr in host_lr], dtype=torch.float32)
            if own and scheduled:
                self.schedule_step += 1
        if not scheduled:
            self.last_lr = None
        # the kernel wrote parameters, gradients and moments through raw pointers: tell autograd's version counters
        # (a graph that still holds the old values must fail loudly, as it does after torch.optim.Adam.step()); a
        # skipped step wrote nothing, which the host cannot know: it bumps all the same
        bump = torch.autograd.graph.increment_version
        for p in own:
            bump(p)
            bump(p.grad)
        for g in keep:
            bump(g)
        self.last_grad_norm = norm
        return loss
