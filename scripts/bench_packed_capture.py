"""Packed batches under one graph capture ("One capture for a data set", packed recipe), and what the
capacity form costs.

Arm "capture": B = 3 clouds per step, point counts drawn per step log-uniformly from 1,276 .. 14,039 (seed 1234, as
scripts/bench_packed.py draws them), capacity = 3 x 14,080 rows.  Step = zero_grad + forward_packed (edge-head dropout
0.1, device seeds) + device WireframeLoss + backward + ClipAdam(capturable).  "Eager": the default model, host point
counts, each batch uploaded and passed as is (a new row layout per list of counts).  "Replay": set_edge_layout("padded"),
device point counts, captured once on static buffers; per step pack_into + target copies + graph.replay(), all inside
the timing.  Device events over --steps steps after --warmup, the protocol of scripts/bench_graphed_loop.py.
The replay is then repeated under the encoder's tail="compute" and tail="skip" (one capture each, the same static
buffers and batches) in --blocks alternating blocks of --block-steps x 16 steps (every block walks all 16 batches), a device event pair per step: the median of
block medians of each, each one's block-to-block spread (max - min of its block medians), their ratio, and
capacity / mean live rows of the batches beside it — the most the encoder's share of the step could gain.

Arm "capacity": counts [4096] x 32 (cfg2's shape), forward + backward: forward_packed on host counts without capacity
against capacity = 131,072 with device counts under tail="compute" and tail="skip" (nothing to skip: what the count costs),
in alternating blocks; the median of block medians of each, their gaps, and the plain and the compute arm's block-to-block
spreads (max - min of block medians).

    python scripts/bench_packed_capture.py [--arms capture,capacity] [--steps 200] [--warmup 5] [--blocks 5] [--out FILE]

Prints one JSON line per arm (and appends them to --out).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "wireframe-3d-prediction_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from losses.WireframeLoss import WireframeLoss  # noqa: E402
from models.PointCloudToWireframe import PointCloudToWireframe  # noqa: E402
from wf3d import config  # noqa: E402
from wf3d.optim import ClipAdam  # noqa: E402
from wf3d.packed import pack, pack_into  # noqa: E402
from wf3d.targets import train_targets  # noqa: E402

LO, HI = 1276, 14039                           # the demo clouds' point counts
KEYS = ("vertices", "vertex_existence", "edge_labels", "vertex_counts")


def capture_arm(steps, warmup, dev, blocks=5, block_steps=10, B=3, V=38, nb=16):
    cap = B * 14080
    rng = np.random.default_rng(1234)
    data = []
    for _ in range(nb):
        pc = np.exp(rng.uniform(np.log(LO), np.log(HI), size=B)).astype(np.int64).tolist()
        cnt = rng.integers(4, V + 1, size=B).tolist()
        vs = [rng.standard_normal((c, 3)).astype(np.float32) for c in cnt]
        es = [np.stack([np.arange(c - 1), np.arange(1, c)], 1) for c in cnt]
        t = train_targets(vs, es, V, device=dev, full_width=True)
        t["clouds"] = [torch.from_numpy(rng.standard_normal((n, 8)).astype(np.float32)) for n in pc]
        t["width"] = max(c * (c - 1) // 2 for c in cnt)
        data.append(t)
    crit = WireframeLoss(vertex_weight=3.0, edge_weight=1.0, existence_weight=1.5, assignment="device")

    def model(layout):
        torch.manual_seed(0)
        m = PointCloudToWireframe(8, V).to(dev).set_dropout(0.1).train().set_edge_layout(layout)
        return m, ClipAdam(m.parameters(), lr=1e-3, weight_decay=1e-6, max_norm=1.0, norm_params=m.parameters, capturable=True)

    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fn):
        for k in range(warmup):
            fn(k)
        torch.cuda.synchronize()
        ev[0].record()
        for k in range(steps):
            fn(k)
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / steps

    m, opt = model("ragged")
    losses = []

    def eager(k):
        bt = data[k % nb]
        points, pc = pack(bt["clouds"])
        opt.zero_grad()
        out = m.forward_packed(points.to(dev), pc, bt["vertex_counts"])
        tg = {key: bt[key] for key in KEYS}
        tg["edge_labels"] = bt["edge_labels"][:, :bt["width"]]
        res = crit(out, tg)
        res["total_loss"].backward()
        opt.step()
        losses.append(res["total_loss"].detach())
    eager_ms = timed(eager)
    finite = bool(torch.isfinite(torch.stack(losses)).all())
    del m, opt

    static = {key: data[0][key].clone() for key in KEYS}
    points = torch.zeros(cap, 8, device=dev)
    counts = torch.zeros(B, dtype=torch.int64, device=dev)
    pack_into(points, counts, data[0]["clouds"])
    status = []

    def captured(tail):
        """One captured step under the encoder's `tail`, on the shared static buffers -> replay(k)."""
        m, opt = model("padded")
        m.set_packed_tail(tail)
        held = {"model": m, "optimizer": opt}          # the graph holds their addresses: they live as long as it does

        def step():
            opt.zero_grad()
            out = m.forward_packed(points, counts, static["vertex_counts"], capacity=cap)
            res = crit(out, static)
            res["total_loss"].backward()
            opt.step()
            held["loss"], held["status"] = res["total_loss"], out["point_status"]

        s = torch.cuda.Stream(dev)
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                step()
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            step()

        def replay(k):
            bt = data[k % nb]
            pack_into(points, counts, bt["clouds"])
            for key in KEYS:
                static[key].copy_(bt[key])
            graph.replay()
            status.append(held["status"].clone())
        return replay, held

    replays = {tail: captured(tail) for tail in ("compute", "skip")}
    replay_ms = timed(replays["compute"][0])
    finite = finite and all(bool(torch.isfinite(h["loss"]).all()) for _, h in replays.values())
    # compute against skip: alternating blocks, every block walks the same batches
    n = block_steps * nb
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    med = {tail: [] for tail in replays}
    for _ in range(blocks):
        for tail, (fn, _) in replays.items():
            torch.cuda.synchronize()
            for k, (a, b) in enumerate(evs):
                a.record()
                fn(k)
                b.record()
            torch.cuda.synchronize()
            med[tail].append(float(np.median([a.elapsed_time(b) for a, b in evs])))
    comp, skip = float(np.median(med["compute"])), float(np.median(med["skip"]))
    spread = {tail: max(v) - min(v) for tail, v in med.items()}
    mean_live = float(np.mean([sum(c.shape[0] for c in bt["clouds"]) for bt in data]))
    finite = finite and all(bool(torch.isfinite(h["loss"]).all()) for _, h in replays.values())
    return {"arm": "capture", "B": B, "V": V, "capacity": cap, "batches": nb, "counts_range": [LO, HI], "steps": steps,
            "dropout": 0.1, "eager_host_counts_ms_per_step": round(eager_ms, 3), "replay_ms_per_step": round(replay_ms, 3),
            "eager_over_replay": round(eager_ms / replay_ms, 2), "blocks": blocks, "steps_per_block": n,
            "replay_tail_compute_ms": round(comp, 3), "compute_block_spread_ms": round(spread["compute"], 3),
            "replay_tail_skip_ms": round(skip, 3), "skip_block_spread_ms": round(spread["skip"], 3),
            "compute_over_skip": round(comp / skip, 3), "mean_live_rows": round(mean_live, 1),
            "capacity_over_mean_live_rows": round(cap / mean_live, 3),
            "skip_faster_by_more_than_twice_the_spread": bool(comp - skip > 2 * spread["compute"]),
            "point_status_or": int(torch.stack(status).max()), "finite_loss": finite, "precision": config.precision()}


def capacity_arm(blocks, steps, warmup, dev, B=32, N=4096, V=64):
    cap = B * N
    torch.manual_seed(0)
    m = PointCloudToWireframe(8, V).to(dev).set_dropout(0.0).train().set_edge_layout("padded")
    g = torch.Generator().manual_seed(1)
    points = torch.randn(cap, 8, generator=g).to(dev)
    host, devc = [N] * B, torch.full((B,), N, dtype=torch.int64, device=dev)
    tc = torch.randint(4, V + 1, (B,), generator=g).to(dev)

    def step(counts, capacity, tail="compute"):
        for p in m.parameters():
            p.grad = None
        out = m.set_packed_tail(tail).forward_packed(points, counts, tc, capacity=capacity)
        (out["vertices"].sum() + out["existence_probabilities"].sum() + out["edge_probs"].sum()).backward()

    arms = {"plain": lambda: step(host, None), "capacity": lambda: step(devc, cap), "skip": lambda: step(devc, cap, "skip")}
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    med = {k: [] for k in arms}
    for _ in range(warmup):
        for fn in arms.values():
            fn()
    for _ in range(blocks):
        for name, fn in arms.items():                  # alternating blocks
            torch.cuda.synchronize()
            for a, b in ev:
                a.record()
                fn()
                b.record()
            torch.cuda.synchronize()
            med[name].append(float(np.median([a.elapsed_time(b) for a, b in ev])))
    plain, capm, skip = (float(np.median(med[k])) for k in ("plain", "capacity", "skip"))
    spread = max(med["plain"]) - min(med["plain"])
    cspread = max(med["capacity"]) - min(med["capacity"])
    return {"arm": "capacity", "B": B, "N": N, "V": V, "capacity": cap, "blocks": blocks, "steps_per_block": steps,
            "plain_packed_ms": round(plain, 3), "plain_block_spread_ms": round(spread, 3), "capacity_ms": round(capm, 3),
            "gap_ms": round(capm - plain, 3), "within_twice_the_spread": bool(abs(capm - plain) <= 2 * spread),
            "capacity_block_spread_ms": round(cspread, 3), "capacity_skip_ms": round(skip, 3),
            "skip_gap_ms": round(skip - capm, 3), "skip_within_twice_the_spread": bool(skip - capm <= 2 * cspread),
            "precision": config.precision()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arms", default="capture,capacity")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--block-steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    config.set_dropout_rng("device")
    dev = torch.device("cuda:0")
    for arm in args.arms.split(","):
        r = capture_arm(args.steps, args.warmup, dev, args.blocks, args.block_steps) if arm == "capture" else \
            capacity_arm(args.blocks, args.block_steps, args.warmup, dev)
        print(json.dumps(r), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
