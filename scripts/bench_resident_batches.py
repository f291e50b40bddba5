"""Preparing one packed batch for a captured step ("One capture for packed batches"): the host recipe
against the resident data set, on the three fixture clouds of tests/golden/building3d (1,276 / 1,504 / 2,479 points; 8 / 4 /
4 wireframe vertices) cycled to B = 3 and B = 32, augmentation on, max_vertices = 16, capacity = the batch's rows rounded
up to a multiple of 256.

Arm "host": `dataset[i]` per sample (file read, normalisation, augmentation) + `collate_packed` + `wf3d.packed.pack_into` +
`wf3d.targets.train_targets(full_width=True)` + the four target `copy_`s into static device buffers.
Arm "resident": `DeviceCloudCache.stage` + `fill` into buffers of the same shapes.
Both: host wall time of one batch's preparation, ended by a synchronize.  2 warm-up batches per arm, then --blocks
alternating blocks of --block-steps batches; the median of block medians of each arm and its block-to-block spread (max -
min of its block medians), the protocol of scripts/bench_packed_capture.py's capacity arm.

"fill": the two launches alone between device events, same blocks; GB/s over the bytes the point launch must move (96 B
per cloud row at 8 columns, 32 B per zero row) beside `roofline.hbm.rows.achieved` of the newest committed
profiles/r*_bench_cfg2.json (bench.py's line: the encoder's row passes at cfg2, hundreds of MB per launch).  At B = 3 and
B = 32 the two launches move 0.5 and 5 MB: --batch-sizes 1024 shows the point launch at a size where bytes count.

    python scripts/bench_resident_batches.py [--blocks 5] [--block-steps 7] [--warmup 2] [--out profiles/r06_resident_batches.jsonl]

--form fixed: FIXED-SIZE batches [B, --num-points, C] of the same clouds ("One capture for fixed-size
batches").  Arm "batch": `cache.batch(idxs)` — per sample an np.random.choice draw and the augmentation draws, three
uploads, one gather launch.  Arm "sampled": `cache.stage` + one replay of a graph captured around `cache.fill` on
`sampled_buffers` (seed draw, sampler, targets) — the augmentation draws and one 40 B + 4 byte copy.  Host wall time per
batch as above, both ended by a synchronize; then the device time of each form's launches between events (--reps
back-to-back launches per reading): the gather kernel on a resident choice table, the sampler kernel, the replayed graph.
GB/s of the two point kernels over B * P * (64 + 32) bytes.  Note that "batch" also builds the host dict fields of
collate_batch (wireframe lists), which "sampled" replaces by device targets: the arms are the two ways to feed a step.

    python scripts/bench_resident_batches.py --form fixed --batch-sizes 32 --num-points 4096 --out profiles/r10_sampled_batches.jsonl

--form epoch: the same fixed-size batches with NOTHING made on the host ("One capture for a data set,
nothing between replays").  Arm "sampled" as above (`cache.stage` + one replay of a graph around `cache.fill`); arm
"epoch": one replay of a graph captured around `cache.fill_epoch` (epoch parameters, sampler, targets) under an
EpochSampler over the same clouds cycled to 4 B members — no draw, no mirror, no copy.  Host wall time per batch of
both, ended by a synchronize, in one alternation; then the device time of each replayed graph (three launches each)
between events over --reps back-to-back replays.

    python scripts/bench_resident_batches.py --form epoch --batch-sizes 32 --num-points 4096 --out profiles/r18_epoch_batches.jsonl

--sampler fps (both forms above): the sampled buffers choose their rows by farthest-point sampling
(`sampled_buffers(..., sampler="fps")`, wf3d_cloud_sample_fps): min(n, P) - 1 dependent rounds per sample instead of one
gather pass, so "sampler", "graph" and the replay arms then show what the fill costs; --longest makes every sample the
longest fixture cloud (2,479 rows).  The GB/s figure of an FPS sampler says nothing: its time is rounds, not bytes.

    python scripts/bench_resident_batches.py --form fixed --sampler fps --batch-sizes 32 --num-points 2560 --out profiles/r19_fps_batches.jsonl

--augment (both forms above): the sampled buffers carry the augmentation extension (`sampled_buffers(..., augment=AUGMENT)`:
anisotropic scale, clipped jitter, point dropout), so the same arms run the `_ext` entry points — per point three 64-bit
hashes for the jitter and one for the dropout on top of the plain gather.  Without it the lines are what they were, plus
"augment": null.

    python scripts/bench_resident_batches.py --form epoch --augment --batch-sizes 32 --num-points 4096 --out profiles/r20_augment_batches.jsonl

Prints one JSON line per batch size and appends them to --out.
"""
import argparse
import glob
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "wireframe-3d-prediction_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from datasets import Building3DReconstructionDataset, DeviceCloudCache  # noqa: E402
from wf3d.packed import pack_into  # noqa: E402
from wf3d.targets import train_targets  # noqa: E402

KEYS = ("vertices", "vertex_existence", "edge_labels", "vertex_counts")
V = 16
AUGMENT = {"scale": (0.8, 1.25), "anisotropic": True, "jitter_sigma": 0.01, "jitter_clip": 0.05, "max_dropout": 0.875}


def sampled_buffers(cache, B, P, args):
    """--augment: with the extension; else exactly the call this script always made"""
    if args.augment:
        return cache.sampled_buffers(B, V, P, sampler=args.sampler, augment=AUGMENT)
    return cache.sampled_buffers(B, V, P, sampler=args.sampler)


def fixture_dataset():
    """the train split's two clouds and the test split's one in one data set, num_points = 0"""
    cfg = types.SimpleNamespace(root_dir=os.path.join(ROOT, "tests", "golden", "building3d"), num_points=0, use_color=True,
                                use_intensity=True, normalize=True, augment=True)
    ds = Building3DReconstructionDataset(cfg, "train")
    other = Building3DReconstructionDataset(cfg, "test")
    ds.pc_files, ds.wireframe_files = ds.pc_files + other.pc_files, ds.wireframe_files + other.wireframe_files
    order = np.argsort([os.path.basename(f) for f in ds.pc_files])
    ds.pc_files, ds.wireframe_files = [ds.pc_files[i] for i in order], [ds.wireframe_files[i] for i in order]
    return ds


def batch_indices(B, ds, cache, args):
    """the fixture clouds cycled to B samples, or (--longest) the longest of them B times"""
    return [int(np.argmax(cache.n))] * B if args.longest else [i % len(ds) for i in range(B)]


def rows_figure():
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_bench_cfg2.json")))
    if not files:
        return None

    def find(o):
        if isinstance(o, dict):
            if isinstance(o.get("hbm"), dict) and "rows" in o["hbm"]:
                return o["hbm"]["rows"].get("achieved")
            o = list(o.values())
        for v in o if isinstance(o, list) else []:
            r = find(v)
            if r is not None:
                return r
        return None
    with open(files[-1]) as f:
        r = find(json.load(f))
    return None if r is None else {"file": os.path.basename(files[-1]), "GB/s": round(float(r), 1)}


def blocks_of(arms, blocks, steps, warmup):
    """{arm: block medians} of the per-call figures fn() returns, in alternating blocks"""
    for fn in arms.values():
        for _ in range(warmup):
            fn()
    med = {k: [] for k in arms}
    for _ in range(blocks):
        for name, fn in arms.items():
            torch.cuda.synchronize()
            med[name].append(float(np.median([fn() for _ in range(steps)])))
    return med


def summary(v, digits=4):
    return {"median": round(float(np.median(v)), digits), "block_spread": round(max(v) - min(v), digits)}


def run(B, ds, cache, dev, args):
    idxs = [i % len(ds) for i in range(B)]
    rows = sum(cache.n[i] for i in idxs)
    cap = -(-rows // 256) * 256
    buf = cache.packed_buffers(B, cap, V)
    points = torch.zeros(cap, cache.ncol, device=dev)
    counts = torch.zeros(B, dtype=torch.int64, device=dev)
    static = {k: torch.zeros_like(buf[k]) for k in KEYS}

    def host():
        t0 = time.perf_counter()
        batch = ds.collate_packed([ds[i] for i in idxs])
        pack_into(points, counts, batch["point_clouds"].split(batch["point_counts"].tolist()))
        t = train_targets(batch["wf_vertices"], batch["wf_edges"], V, full_width=True)
        for k in KEYS:
            static[k].copy_(t[k])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def resident():
        t0 = time.perf_counter()
        cache.stage(buf, idxs)
        cache.fill(buf)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def fill():
        ev[0].record()
        cache.fill(buf)
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1])

    np.random.seed(0)
    med = blocks_of({"host": host, "resident": resident}, args.blocks, args.block_steps, args.warmup)
    # the two arms built the same batch last (same draws are not needed for that: compare what does not depend on them)
    same = bool(torch.equal(counts, buf["point_counts"]) and torch.equal(static["edge_labels"], buf["edge_labels"])
                and torch.equal(static["vertex_counts"], buf["vertex_counts"]))
    fmed = blocks_of({"fill": fill}, args.blocks, args.block_steps, args.warmup)["fill"]
    nbytes = rows * cache.ncol * 12 + (cap - rows) * cache.ncol * 4
    fill_ms = float(np.median(fmed))
    h, r = summary(med["host"]), summary(med["resident"])
    return {"bench": "resident_batches", "B": B, "rows": rows, "capacity": cap, "max_vertices": V, "columns": cache.ncol,
            "blocks": args.blocks, "steps_per_block": args.block_steps, "host_prepare_ms": h, "resident_prepare_ms": r,
            "host_over_resident": round(h["median"] / r["median"], 1), "h2d_bytes_resident": 40 * B + 4,
            "h2d_bytes_host": cap * cache.ncol * 4 + 8 * B + sum(static[k].numel() * static[k].element_size() for k in KEYS),
            "same_counts_and_labels": same, "fill_ms": summary(fmed), "fill_point_bytes": nbytes,
            "fill_GB/s": round(nbytes / fill_ms / 1e6, 1), "row_passes": rows_figure()}


def run_fixed(B, ds, cache, dev, args):
    from wf3d import _lib
    from wf3d.ops import _stream
    P = args.num_points
    ds.num_points = P
    idxs = batch_indices(B, ds, cache, args)
    buf = sampled_buffers(cache, B, P, args)
    np.random.seed(0)
    cache.stage(buf, idxs)
    cache.fill(buf)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cache.fill(buf)

    def batch():
        t0 = time.perf_counter()
        cache.batch(idxs)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def sampled():
        t0 = time.perf_counter()
        cache.stage(buf, idxs)
        graph.replay()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    med = blocks_of({"batch": batch, "sampled": sampled}, args.blocks, args.block_steps, args.warmup)
    lib = _lib.load()
    ids = torch.tensor(idxs, dtype=torch.int32, device=dev)
    choice = torch.from_numpy(np.stack([np.random.choice(cache.n[i], P, replace=cache.n[i] < P) for i in idxs]).astype(np.int32)).to(dev)
    aug = torch.from_numpy(cache._block_views(buf["params_host"], B)[0].copy()).to(dev)
    out = torch.empty_like(buf["points"])
    ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(launch):
        def fn():
            ev[0].record()
            for _ in range(args.reps):
                launch()
            ev[1].record()
            torch.cuda.synchronize()
            return ev[0].elapsed_time(ev[1]) * 1e3 / args.reps
        return fn

    dmed = blocks_of({"gather": timed(lambda: _lib.check(lib.wf3d_cloud_sample(
                          cache.norm.data_ptr(), cache.first.data_ptr(), ids.data_ptr(), choice.data_ptr(), aug.data_ptr(), B, P,
                          cache.ncol, out.data_ptr(), _stream()), "cloud_sample")),
                      "sampler": timed(lambda: cache._sample(buf["params"], buf["sample_words"], out,
                                                             buf if args.sampler == "fps" else None,
                                                             *((buf["aug_ext"],) if args.augment else ()))),
                      "graph": timed(graph.replay)}, args.blocks, args.block_steps, args.warmup)
    nbytes = B * P * cache.ncol * 12
    b, r = summary(med["batch"]), summary(med["sampled"])
    dev_us = {k: summary(v, 2) for k, v in dmed.items()}
    return {"bench": "sampled_batches", "sampler": args.sampler, "augment": AUGMENT if args.augment else None, "B": B, "num_points": P, "columns": cache.ncol, "max_vertices": V,
            "cloud_rows": sorted(set(cache.n[i] for i in idxs)), "blocks": args.blocks, "steps_per_block": args.block_steps,
            "reps": args.reps, "batch_ms": b, "sampled_ms": r, "batch_over_sampled": round(b["median"] / r["median"], 2),
            "h2d_bytes_batch": B * P * 4 + 36 * B, "h2d_bytes_sampled": 40 * B + 4, "device_us": dev_us, "point_bytes": nbytes,
            "gather_GB/s": round(nbytes / dev_us["gather"]["median"] / 1e3, 1),
            "sampler_GB/s": round(nbytes / dev_us["sampler"]["median"] / 1e3, 1)}


def run_epoch(B, ds, cache, dev, args):
    """--form epoch: the stage-plus-replay arm of --form fixed beside one replay of a graph captured around
    cache.fill_epoch with NOTHING else per batch, in one session and one alternation"""
    P = args.num_points
    ds.num_points = P
    idxs = batch_indices(B, ds, cache, args)
    members = batch_indices(4 * B, ds, cache, args)                # four steps per epoch over the same clouds
    sampler = cache.epoch_sampler(B, members, seed=0)
    graphs, bufs = {}, {}
    np.random.seed(0)
    for name in ("sampled", "epoch"):
        buf = bufs[name] = sampled_buffers(cache, B, P, args)
        fill = (lambda b=buf: cache.fill(b)) if name == "sampled" else (lambda b=buf: cache.fill_epoch(b, sampler))
        if name == "sampled":
            cache.stage(buf, idxs)
        fill()
        torch.cuda.synchronize()
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            fill()

    def sampled():
        t0 = time.perf_counter()
        cache.stage(bufs["sampled"], idxs)
        graphs["sampled"].replay()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def epoch():
        t0 = time.perf_counter()
        graphs["epoch"].replay()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    t_before = int(sampler.get_state()[1])
    med = blocks_of({"sampled": sampled, "epoch": epoch}, args.blocks, args.block_steps, args.warmup)
    batches = int(sampler.get_state()[1]) - t_before
    ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(launch):
        def fn():
            ev[0].record()
            for _ in range(args.reps):
                launch()
            ev[1].record()
            torch.cuda.synchronize()
            return ev[0].elapsed_time(ev[1]) * 1e3 / args.reps
        return fn

    dmed = blocks_of({"fill_graph": timed(graphs["sampled"].replay), "fill_epoch_graph": timed(graphs["epoch"].replay)},
                     args.blocks, args.block_steps, args.warmup)
    # the walk went where the specification says
    t = int(sampler.get_state()[1])
    cloud = cache._block_views(bufs["epoch"]["params"].cpu(), B)[1]
    s, e = summary(med["sampled"]), summary(med["epoch"])
    return {"bench": "epoch_batches", "sampler": args.sampler, "augment": AUGMENT if args.augment else None, "B": B, "num_points": P, "columns": cache.ncol, "max_vertices": V,
            "cloud_rows": sorted(set(cache.n[i] for i in idxs)), "members": len(members),
            "steps_per_epoch": sampler.steps_per_epoch, "blocks": args.blocks, "steps_per_block": args.block_steps, "reps": args.reps,
            "stage_replay_ms": s, "epoch_replay_ms": e, "stage_replay_over_epoch": round(s["median"] / e["median"], 2),
            "h2d_bytes_stage": 40 * B + 4, "h2d_bytes_epoch": 0, "host_draws_epoch": 0,
            "batches_walked": batches == args.blocks * args.block_steps + args.warmup,
            "last_batch_is_specified": cloud.tolist() == sampler.batch_at(t - 1)["cloud"].tolist(),
            "device_us": {k: summary(v, 2) for k, v in dmed.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--block-steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch-sizes", default="3,32")
    ap.add_argument("--form", choices=("packed", "fixed", "epoch"), default="packed")
    ap.add_argument("--num-points", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sampler", choices=("device", "fps"), default="device", help="--form fixed / epoch: how the rows are chosen")
    ap.add_argument("--augment", action="store_true", help="--form fixed / epoch: the sampled buffers carry the augmentation extension")
    ap.add_argument("--longest", action="store_true", help="--form fixed / epoch: every sample is the longest fixture cloud")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r06_resident_batches.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ds = fixture_dataset()
    cache = DeviceCloudCache(ds, dev)
    for B in (int(b) for b in args.batch_sizes.split(",")):
        r = {"fixed": run_fixed, "epoch": run_epoch, "packed": run}[args.form](B, ds, cache, dev, args)
        print(json.dumps(r), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
