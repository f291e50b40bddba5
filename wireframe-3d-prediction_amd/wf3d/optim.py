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
a graph would freeze."""
import ctypes

import torch

from . import _lib
from ._lib import check
from .ops import _stream


class ClipAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_norm=None, norm_params=None,
                 capturable=False):
        if not isinstance(capturable, bool):
            raise TypeError(f"ClipAdam: capturable must be a bool, got {type(capturable).__name__}")
        if torch.is_tensor(lr):
            if not capturable:
                raise ValueError("ClipAdam: a tensor lr needs capturable=True (a non-capturable step reads lr on the host)")
            if lr.numel() != 1 or lr.dim() != 0 or lr.dtype != torch.float32:
                raise ValueError("ClipAdam: a tensor lr must be a 0-d fp32 tensor")
            if float(lr) < 0:
                raise ValueError("ClipAdam: bad hyper-parameters")
        elif lr < 0:
            raise ValueError("ClipAdam: bad hyper-parameters")
        if eps < 0 or not (0 <= betas[0] < 1 and 0 <= betas[1] < 1) or weight_decay < 0:
            raise ValueError("ClipAdam: bad hyper-parameters")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, capturable=capturable))
        if len(self.param_groups) != 1:
            raise ValueError("ClipAdam: one parameter group (the global gradient norm spans all tensors of one launch)")
        self.max_norm = max_norm
        self.capturable = capturable
        self._norm_params = norm_params
        self.last_grad_norm = None          # device scalar: pre-clip global L2 norm of the last step

    def load_state_dict(self, state_dict):
        # the saved group's "capturable" (torch.optim.Adam writes one) does not change how this optimizer steps; step
        # counters of the other layout are converted at the next step()
        super().load_state_dict(state_dict)
        self.param_groups[0]["capturable"] = self.capturable

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        group = self.param_groups[0]
        capturable = self.capturable
        capturing = torch.cuda.is_current_stream_capturing()
        if not capturable and capturing:
            raise RuntimeError("ClipAdam: step() inside a CUDA graph capture needs ClipAdam(..., capturable=True): the "
                               "non-capturable step reads its step counter and lr on the host, which a graph would freeze")
        own = [p for p in group["params"] if p.grad is not None]
        own_ids = {id(p) for p in group["params"]}
        extra = []
        if self._norm_params is not None:
            src = self._norm_params() if callable(self._norm_params) else self._norm_params
            extra = [p for p in src if id(p) not in own_ids and p.grad is not None]
        if not own and not extra:
            return loss
        # validate everything and collect the pointers FIRST; the per-parameter step counters are advanced only after the
        # launch has been accepted, so that a failed step leaves the optimizer where it was and can simply be retried
        steps = set()
        P, G, M, V, N = [], [], [], [], []
        keep = []
        for p in own:
            g = p.grad
            if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and g.is_cuda and g.dtype == torch.float32):
                raise RuntimeError("ClipAdam: contiguous fp32 CUDA parameters (and fp32 CUDA gradients) only")
            st = self.state[p]
            if capturable:
                # no device step is read here: only whether the state exists (a parameter that first gets a gradient
                # after the others have stepped would start at step 1 beside them)
                steps.add(bool(st))
                if capturing and not st:
                    raise RuntimeError("ClipAdam(capturable=True): run one step before the capture (it creates the state)")
            else:
                steps.add(int(st["step"]) + 1 if st else 1)
        for p in extra:
            g = p.grad
            if not (g.is_cuda and g.dtype == torch.float32):
                raise RuntimeError("ClipAdam: the clip-only tensors of norm_params need fp32 CUDA gradients "
                                   f"(got {g.dtype} on {g.device})")
        if len(steps) > 1:
            raise RuntimeError("ClipAdam: parameters are at different Adam steps (a parameter without gradient in an earlier step); "
                               "use torch.optim.Adam for such models")
        step = steps.pop() if steps and not capturable else 1      # the host step (capturable: read on the device)
        lr = group["lr"]
        if torch.is_tensor(lr) and not (capturable and lr.is_cuda and lr.dtype == torch.float32 and lr.dim() == 0):
            raise RuntimeError("ClipAdam: a tensor lr must be a 0-d fp32 CUDA tensor, with capturable=True")
        S = []
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
        dev = (own or extra)[0].device
        nws = lib.wf3d_clip_adam_ws_floats(numel, n)
        ws = torch.empty(nws, dtype=torch.float32, device=dev)
        norm = torch.empty((), dtype=torch.float32, device=dev)
        b1, b2 = group["betas"]
        if capturable:
            # step counters and a tensor lr are read (and the counters advanced) on the device
            lr_dev = lr.data_ptr() if torch.is_tensor(lr) else None
            check(lib.wf3d_clip_adam_step_dev(vp(*P), vp(*G), vp(*M), vp(*V), vp(*S), numel, n, float(self.max_norm or 0.0),
                                              0.0 if lr_dev else float(lr), lr_dev, float(b1), float(b2), float(group["eps"]),
                                              float(group["weight_decay"]), ws.data_ptr(), nws, norm.data_ptr(), _stream()),
                  "clip_adam_step_dev")
        else:
            check(lib.wf3d_clip_adam_step(vp(*P), vp(*G), vp(*M), vp(*V), numel, n, float(self.max_norm or 0.0), float(lr),
                                          float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]), step,
                                          ws.data_ptr(), nws, norm.data_ptr(), _stream()), "clip_adam_step")
            for p in own:
                self.state[p]["step"] += 1
        # the kernel wrote parameters, gradients and moments through raw pointers: tell autograd's version counters
        # (a graph that still holds the old values must fail loudly, as it does after torch.optim.Adam.step())
        bump = torch.autograd.graph.increment_version
        for p in own:
            bump(p)
            bump(p.grad)
        for g in keep:
            bump(g)
        self.last_grad_norm = norm
        return loss
