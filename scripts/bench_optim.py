"""Row f-2 baseline: GPU time of train.py's step tail (clip_grad_norm_ + Adam.step + zero_grad) for this model."""
import os, sys, statistics
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "wireframe-3d-prediction_amd"))
import torch
from models.PointCloudToWireframe import PointCloudToWireframe
dev = torch.device("cuda:0")
torch.manual_seed(0)
model = PointCloudToWireframe(input_dim=8, max_vertices=64).to(dev)
model.vertex_predictor.ensure_point_pool_proj(1024, dev)
params = [p for p in model.parameters()]
for p in params:
    p.grad = torch.randn_like(p) * 1e-3
print("tensors", len(params), "elements", sum(p.numel() for p in params))


def timeit(fn, n=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


for foreach in (None, False):
    opt = torch.optim.Adam(params, lr=1e-3, weight_decay=1e-6, foreach=foreach)
    t_clip = timeit(lambda: torch.nn.utils.clip_grad_norm_(params, max_norm=1.0, foreach=foreach))
    t_step = timeit(lambda: opt.step())
    print(f"foreach={foreach}: clip_grad_norm_ {t_clip:.3f} ms, Adam.step {t_step:.3f} ms")
try:
    opt = torch.optim.Adam(params, lr=1e-3, weight_decay=1e-6, fused=True)
    print(f"fused=True: Adam.step {timeit(lambda: opt.step()):.3f} ms")
except Exception as e:
    print("fused Adam unavailable:", repr(e)[:120])
from wf3d.optim import ClipAdam
opt = ClipAdam(params[:-2], lr=1e-3, weight_decay=1e-6, max_norm=1.0, norm_params=lambda: params)   # last two = the lazy layer: clip only
print(f"wf3d.optim.ClipAdam (clip + Adam, 2 launches): {timeit(lambda: opt.step()):.3f} ms "
      f"(0.99 GB moved -> {0.99 / timeit(lambda: opt.step()) :.2f} TB/s)")
# the same tensors in two parameter groups (matrices; gains and biases without decay): the grouped launches carry 48
# tensors each instead of 80, so 78 tensors + 2 clip-only take 2 Adam launches where one group takes 1
own = params[:-2]
two = ClipAdam([dict(params=[p for p in own if p.dim() > 1]), dict(params=[p for p in own if p.dim() <= 1], weight_decay=0.0)],
               lr=1e-3, weight_decay=1e-6, max_norm=1.0, norm_params=lambda: params)
for _ in range(3):                                       # alternated, so that a drift shows in both arms
    print(f"ClipAdam one group {timeit(lambda: opt.step()):.3f} ms   two groups {timeit(lambda: two.step()):.3f} ms")


def host_ms(fn, n=20):
    """The call alone, on an idle device: what the host spends before it returns."""
    import time
    ts = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter(); fn(); ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def back_to_back_ms(fn, n=50):
    """n steps issued without waiting: per step, the larger of the host's and the device's time."""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


for name, o in (("one group", opt), ("two groups", two)):
    print(f"ClipAdam {name}: host {host_ms(o.step):.3f} ms, back to back {back_to_back_ms(o.step):.3f} ms per step")


# The capturable grouped step on the same two groups, alone, with a schedule (one small launch more) and with averaged
# weights (40 B per parameter instead of 32), alternated in one run; the plain arm's spread over the rounds is the
# yardstick for the other two.  A report, not a gate.
def capturable(**kw):
    return ClipAdam([dict(params=[p for p in own if p.dim() > 1]), dict(params=[p for p in own if p.dim() <= 1], weight_decay=0.0)],
                    lr=1e-3, weight_decay=1e-6, max_norm=1.0, norm_params=lambda: params, capturable=True, **kw)


n_own = sum(p.numel() for p in own)
arms = (("plain", capturable(), 32),
        ("schedule", capturable(lr_schedule=dict(warmup_steps=500, warmup_start=0.01, decay="cosine", decay_steps=20000, min_factor=0.01)), 32),
        ("ema", capturable(ema_decay=0.999, ema_warmup=True), 40))
ms = {name: [] for name, _, _ in arms}
for _ in range(5):
    for name, o, _ in arms:
        ms[name].append(timeit(o.step))
for name, _, nbytes in arms:
    best = statistics.median(ms[name])
    print(f"capturable two groups, {name}: {best:.3f} ms (rounds {' '.join(f'{t:.3f}' for t in ms[name])}), "
          f"{nbytes} B x {n_own} parameters -> {nbytes * n_own / best / 1e9:.2f} TB/s")
spread = max(ms["plain"]) - min(ms["plain"])
print(f"plain arm's spread over its rounds: {spread:.3f} ms; schedule - plain {statistics.median(ms['schedule']) - statistics.median(ms['plain']):+.3f} ms; "
      f"ema - plain {statistics.median(ms['ema']) - statistics.median(ms['plain']):+.3f} ms")
