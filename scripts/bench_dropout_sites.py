#!/usr/bin/env python3
"""Cost of train-mode dropout at the encoder's and the vertex head's sites: a training step (forward + backward, bf16x3)
at cfg2 (B = 32, N = 4096, V = 64; the edge head's four sites at their default p = 0.1 throughout), four ways.

  off       every encoder / vertex-head site at p = 0: the step bench.py times
  encoder   p at the four encoder sites (mlp[3], [7], [11], [15]): masks in the fused first layer, the three ln_prep
            passes and the four LayerNorm backward passes
  vertex    p at the four vertex-head sites: B = 32 leaves the M <= 32 weight-streaming kernels for the generic GEMM
            route (the skinny kernels draw no masks), so this figure is mostly the price of that route, not of the masks
  both

Each form against `off` in the same process: blocks of --steps timed steps alternate between the forms, a block's figure
is its median, a form's the median of its block medians, with the spread (max - min) of the block medians beside it.
HIP events around each step, warm-up first.  Prints one JSON line (--out FILE appends it there too)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "wireframe-3d-prediction_amd"))
import torch  # noqa: E402
from models.PointCloudToWireframe import PointCloudToWireframe  # noqa: E402
from wf3d import config  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=7, help="timed steps per block (its median is one figure)")
ap.add_argument("--blocks", type=int, default=5, help="blocks per form, alternating between the forms")
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--p", type=float, default=0.1)
ap.add_argument("--rng", choices=config.DROPOUT_RNGS, default="host")
ap.add_argument("--out", default=None)
args = ap.parse_args()

dev = torch.device("cuda:0")
B, N, V = 32, 4096, 64
config.set_precision("bf16x3")
config.set_dropout_rng(args.rng)
torch.manual_seed(1234)
model = PointCloudToWireframe(8, V).to(dev).train()
g = torch.Generator().manual_seed(1)
x = torch.randn(B, N, 8, generator=g).to(dev)
vcounts = torch.randint(4, V + 1, (B,), generator=g)
vcounts[0] = V
vcounts = vcounts.to(dev)
cot = {}

FORMS = {"off": (0.0, 0.0), "encoder": (args.p, 0.0), "vertex": (0.0, args.p), "both": (args.p, args.p)}


def step(form):
    pe, pv = FORMS[form]
    model.set_encoder_dropout(pe).set_vertex_dropout(pv)
    out = model(x, vcounts)
    if not cot:
        cot.update({k: torch.randn_like(out[k]) for k in ("vertices", "existence_probabilities", "edge_probs")})
    sum((out[k] * c).sum() for k, c in cot.items()).backward()


def timed(form):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    model.zero_grad(set_to_none=True)
    e0.record()
    step(form)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


for form in FORMS:
    for _ in range(args.warmup):
        timed(form)
meds = {n: [] for n in FORMS}
for _ in range(args.blocks):
    for form in FORMS:
        meds[form].append(statistics.median(timed(form) for _ in range(args.steps)))
off = statistics.median(meds["off"])
res = {"bench": "dropout_sites", "config": "cfg2", "B": B, "N": N, "V": V, "precision": "bf16x3", "p": args.p, "rng": args.rng,
       "steps": args.steps, "blocks": args.blocks}
for form, m in meds.items():
    t = statistics.median(m)
    res[form] = {"ms_per_step": t, "spread_ms": max(m) - min(m), "blocks_ms": m, "over_off_ms": t - off,
                 "over_off_pct": 100.0 * (t - off) / off}
line = json.dumps(res)
print(line)
if args.out:
    with open(args.out, "a") as f:
        f.write(line + "\n")
