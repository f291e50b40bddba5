#!/usr/bin/env python3
"""Packed point-cloud batches: a training step (forward + backward, bf16x3) on clouds of different lengths, three ways.

  packed   forward_packed on the clouds concatenated along the point axis (M = sum N_b rows, padded to a multiple of 256)
  padded   forward on the batch zero-padded to its longest cloud (B * max N_b rows) — a different result, see DESIGN §4
  loop     B forward calls at B = 1, one per cloud

B = 32, V = 64; the point counts are drawn once (seed 1234), uniform in log-space over the demo tiles' 1,276 .. 14,039.
Then, at equal lengths ([4096] * 32, cfg2's shape), the packed step against the dense step of the same build, alternating,
with the run-to-run spread of the dense figure; and the segmented pool's forward alone beside the dense pool's at the same
bytes.  HIP events around each step, warm-up, medians.  Prints one JSON line (--out FILE appends it there too).
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "wireframe-3d-prediction_amd"))
import torch  # noqa: E402
from models.PointCloudToWireframe import PointCloudToWireframe  # noqa: E402
from wf3d import config, ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=7, help="timed steps per block (its median is one figure)")
ap.add_argument("--blocks", type=int, default=5, help="blocks per form, alternating between the forms")
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=None)
args = ap.parse_args()

dev = torch.device("cuda:0")
B, V, N_LO, N_HI = 32, 64, 1276, 14039
config.set_precision("bf16x3")
torch.manual_seed(1234)
model = PointCloudToWireframe(8, V).to(dev)
model.train()
g = torch.Generator().manual_seed(1234)
u = torch.rand(B, generator=g)
pcounts = [int(round(math.exp(math.log(N_LO) + float(t) * (math.log(N_HI) - math.log(N_LO))))) for t in u]
vcounts = torch.randint(4, V + 1, (B,), generator=g)
vcounts[0] = V
vcounts_host = vcounts.clone()              # the B = 1 loop passes host counts: no device -> host read per call
vcounts = vcounts.to(dev)
cot = {}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    model.zero_grad(set_to_none=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def backward(tag, out):
    if tag not in cot:
        cot[tag] = {k: torch.randn_like(out[k]) for k in ("vertices", "existence_probabilities", "edge_probs")}
    sum((out[k] * c).sum() for k, c in cot[tag].items()).backward()


def compare(forms):
    """{name: fn} -> {name: (median of the block medians, max - min of them, the block medians)}; blocks alternate."""
    for fn in forms.values():
        for _ in range(args.warmup):
            timed(fn)
    meds = {n: [] for n in forms}
    for _ in range(args.blocks):
        for n, fn in forms.items():
            meds[n].append(statistics.median(timed(fn) for _ in range(args.steps)))
    return {n: (statistics.median(m), max(m) - min(m), m) for n, m in meds.items()}


def make(counts):
    gen = torch.Generator().manual_seed(1)
    clouds = [torch.randn(n, 8, generator=gen) for n in counts]
    points = torch.cat(clouds).to(dev)
    nmax = max(counts)
    xpad = torch.zeros(len(counts), nmax, 8)
    for b, c in enumerate(clouds):
        xpad[b, :c.shape[0]] = c
    return [c.to(dev) for c in clouds], points, xpad.to(dev)


res = {"bench": "packed", "B": B, "V": V, "precision": "bf16x3", "steps": args.steps, "blocks": args.blocks}

# --- ragged counts: packed / zero-padded / loop of B = 1
clouds, points, xpad = make(pcounts)
lay = ops.PackedLayout.get(pcounts, dev)
M = lay.M


def loop():
    for b, c in enumerate(clouds):
        backward(("loop", b), model(c[None], vcounts_host[b:b + 1]))


r = compare({"packed": lambda: backward("packed", model.forward_packed(points, pcounts, vcounts)),
             "padded": lambda: backward("padded", model(xpad, vcounts)),
             "loop": loop})
res["ragged"] = {"point_counts": pcounts, "M": M, "M_pad": lay.M_pad, "padded_rows": B * max(pcounts),
                 "row_ratio_padded_over_packed": B * max(pcounts) / lay.M_pad,
                 **{n: {"ms_per_step": t, "spread_ms": s, "points_per_s": M / t * 1e3} for n, (t, s, _) in r.items()}}
res["ragged"]["speedup_over_padded"] = r["padded"][0] / r["packed"][0]
res["ragged"]["speedup_over_loop"] = r["loop"][0] / r["packed"][0]
del clouds, points, xpad
cot.clear()

# --- equal lengths (cfg2): packed against dense, same build, same run
N = 4096
x = torch.randn(B, N, 8, generator=torch.Generator().manual_seed(1)).to(dev)
eq = [N] * B
r = compare({"dense": lambda: backward("dense", model(x, vcounts)),
             "packed": lambda: backward("dense", model.forward_packed(x.view(B * N, 8), eq, vcounts))})
gap, spread = r["packed"][0] - r["dense"][0], r["dense"][1]
res["equal_lengths"] = {"N": N, "dense_ms": r["dense"][0], "dense_spread_ms": spread, "dense_blocks_ms": r["dense"][2],
                        "packed_ms": r["packed"][0], "packed_blocks_ms": r["packed"][2], "gap_ms": gap,
                        "within_twice_the_dense_spread": bool(gap <= 2 * spread)}
cot.clear()

# --- the pool's forward alone: achieved GB/s, Infinity Cache flushed before each launch (scripts/bench_pool.py)
flush = torch.empty(1 << 29, dtype=torch.uint8, device=dev)
C = 512


def pool_gbs(fn, nbytes):
    ts = []
    for _ in range(12):
        flush.zero_()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    t = statistics.median(ts[2:])
    return {"us": t * 1e3, "GB/s": nbytes / t / 1e6}


pf = torch.randn(B * N, C, device=dev)
valid = (torch.rand(B * N, device=dev) > 0.1).float()
lay_eq = ops.PackedLayout.get(eq, dev)
res["pool_fwd"] = {"bytes": pf.numel() * 4,
                   "dense": pool_gbs(lambda: ops.pool4_fwd(pf.view(B, N, C), valid, packed=True), pf.numel() * 4),
                   "segmented_equal_lengths": pool_gbs(lambda: ops.pool4_seg_fwd(pf, valid, lay_eq), pf.numel() * 4)}
pf = torch.randn(lay.M_pad, C, device=dev)
valid = (torch.rand(lay.M_pad, device=dev) > 0.1).float()
res["pool_fwd"]["segmented_ragged"] = {"bytes": M * C * 4, **pool_gbs(lambda: ops.pool4_seg_fwd(pf, valid, lay), M * C * 4)}
dm = torch.randn(B, 2 * C, device=dev)
po = ops.pool4_seg_fwd(pf, valid, lay)
res["pool_bwd_sx8"] = {"segmented_ragged": {"bytes": lay.M_pad * C * 4, **pool_gbs(
    lambda: ops.pool4_seg_bwd(valid, po.cnt, po.arg_m, po.arg_u, dm[:, :C], dm[:, C:], dm[:, C:], dm[:, :C], None, lay, C, sx8=True),
    lay.M_pad * C * 4)}}

line = json.dumps(res)
print(line)
if args.out:
    with open(args.out, "a") as f:
        f.write(line + "\n")
