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
over groups in any way give the norm — and, with equal hyper-parameters, the step — of one group, bit for bit."""
import ctypes

import torch

from . import _lib
from ._lib import check
from .ops import _stream

MAX_GROUPS = 16     # the kernel-argument table of wf3d_clip_adam_step_groups


class ClipAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_norm=None, norm_params=None,
                 capturable=False, decoupled_weight_decay=False, skip_nonfinite=False):
        for name, flag in (("capturable", capturable), ("skip_nonfinite", skip_nonfinite)):
            if not isinstance(flag, bool):
                raise TypeError(f"ClipAdam: {name} must be a bool, got {type(flag).__name__}")
        if skip_nonfinite and not capturable:
            raise ValueError("ClipAdam: skip_nonfinite=True needs capturable=True (the non-capturable step advances its step "
                             "counters on the host, which cannot know that the device skipped)")
        self.capturable = capturable        # add_param_group (called by the base constructor) reads it
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                                      decoupled_weight_decay=decoupled_weight_decay, capturable=capturable))
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
            group.setdefault("decoupled_weight_decay", self.defaults["decoupled_weight_decay"])
        # the one place where the host may look at the loaded counters
        self._lockstep = len({float(st["step"]) for st in self.state.values() if "step" in st}) <= 1

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
                  and one_step)
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
        P, G, M, V, N = [], [], [], [], []
        keep = []
        for p in own:
            g = p.grad
            if not g.is_contiguous():
                g = p.grad = g.contiguous()
            st = self.state[p]
            if not st:
                st["step"] = torch.zeros((), dtype=torch.float32, device=p.device) if capturable else torch.tensor(0.0)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
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
            lr = group["lr"]
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
            lrs = [group["lr"] for group in groups]
            lr_dev = (ctypes.c_void_p * ng)(*[lr.data_ptr() if torch.is_tensor(lr) else None for lr in lrs])
            check(lib.wf3d_clip_adam_step_groups(
                vp(*P), vp(*G), vp(*M), vp(*V), numel, (ctypes.c_int * n)(*K), vp(*S) if capturable else None, n,
                dbl(*[0.0 if torch.is_tensor(lr) else float(lr) for lr in lrs]), lr_dev,
                dbl(*[float(group["betas"][0]) for group in groups]), dbl(*[float(group["betas"][1]) for group in groups]),
                dbl(*[float(group["eps"]) for group in groups]), dbl(*[float(group["weight_decay"]) for group in groups]),
                integer(*[int(group.get("decoupled_weight_decay", False)) for group in groups]),
                integer(*[next(iter(s)) if s else 1 for s in gsteps]), ng, max_norm,
                _lib.DEFINES["WF3D_ADAM_SKIP_NONFINITE"] if self.skip_nonfinite else 0,
                self.skipped_steps.data_ptr() if self.skip_nonfinite else None, ws.data_ptr(), nws, norm.data_ptr(), _stream()),
                "clip_adam_step_groups")
        if not capturable:
            for p in own:
                self.state[p]["step"] += 1
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
