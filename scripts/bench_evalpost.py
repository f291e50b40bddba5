"""Evaluation post-processing per batch (DESIGN.md §5 "Evaluation post-processing"): the every-candidate path against the
compacted one, on synthetic predictions of B = 32 samples at V = 64 and V = 256 vertices.

Every sample has counts = V and keeps about 1.5 V edges: the 18 edges of a fixed 12-vertex label wireframe (a hexagonal
prism), whose vertices are the first 12 predicted ones plus N(0, 0.02) noise, and random other pairs.  Two layouts of the
predictions dict: "ragged" (`edge_indices` = edge_index_lists) and "padded" (device `edge_counts` and a fresh
EdgeIndexLists per batch, as every padded forward returns one).

Pairs of arms, old against new:
    wireframes      wf3d.postprocess.wireframes_from_predictions   against   wireframes_compact
    evaluate        evaluate_batch(compact=False)                  against   evaluate_batch(compact=True)
both with eval.ap_calculator.set_device(cuda:0), so that the old evaluate arm is the per-sample device Hausdorff call.  The
old arms are the functions as they were before the compact path existed (compact=False is that code path unchanged).

Host wall time of one batch, ended by the results being on the host (all four functions return host data).  The protocol
of scripts/bench_resident_batches.py: 2 warm-up batches per arm, then --blocks alternating blocks of --block-steps
batches; the median of block medians of each arm and its block-to-block spread (max - min of its block medians).

    python scripts/bench_evalpost.py [--blocks 5] [--block-steps 7] [--warmup 2] [--out profiles/r13_evalpost.jsonl]

Prints one JSON line per arm and appends them to --out.  `d2h_bytes` are the formulas' values, not measurements:
old B (3 V + 7 max_e) 4; new (B + 1) 4 + 12 B V + 36 K.

    python scripts/bench_evalpost.py --what metrics [--out profiles/r15_evalmetrics.jsonl]

measures evaluate_batch(compact=True) three ways in the same alternating blocks: "compact" (metrics="host": the yardstick),
"device" (metrics="device", the EvalLabels built inside the timed call) and "device_labels" (an EvalLabels built once,
outside).  Then one worst-case row: V = 64 with every one of the 2016 candidates kept, against a label of 120 vertices
and 300 edges (few blocks: the host arm solves 32 assignments of 2016 x 300 per batch).

    python scripts/bench_evalpost.py --what decode [--out profiles/r20_decode.jsonl]

measures evaluate_batch(compact=True, metrics="device", labels=...) without and with `decode` (wf3d_wireframe_decode in
front, wf3d_eval_metrics_nv behind) on the same predictions, padded layout: "undecoded" (decode=None: the call as it was
before decoding existed), "decoded" (every slot alive, merge_radius 0.05 merges nothing: the same wireframes, so the
difference is the cost of the step) and "decoded_sparse" (the 12 label slots and a quarter of the others alive: what the
step saves downstream).  Existence values come from a generator of their own, so the predictions are those of --what metrics.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "wireframe-3d-prediction_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from eval import ap_calculator as ap  # noqa: E402
from wf3d import postprocess  # noqa: E402
from wf3d.functional import EdgeIndexLists, edge_index_lists  # noqa: E402

B = 32


def label_wireframe():
    """12 vertices, 18 edges: two hexagons (z = 0 and z = 3, the upper one turned by 0.2 rad so that no two label
    vertices share all but one coordinate by construction) and the six uprights."""
    a = np.arange(6) * (np.pi / 3)
    low = np.stack((4 * np.cos(a), 4 * np.sin(a), np.zeros(6)), axis=1)
    top = np.stack((3 * np.cos(a + 0.2), 3 * np.sin(a + 0.2), np.full(6, 3.0)), axis=1)
    edges = [(i, (i + 1) % 6) for i in range(6)] + [(6 + i, 6 + (i + 1) % 6) for i in range(6)] + [(i, 6 + i) for i in range(6)]
    return np.concatenate((low, top)).astype(np.float32), np.array(sorted((min(e), max(e)) for e in edges), dtype=np.int64)


def synthetic(V, gen, dev):
    gt_v, gt_e = label_wireframe()
    max_e = V * (V - 1) // 2
    verts = gen.uniform(-8, 8, (B, V, 4)).astype(np.float32)
    verts[:, :12, :3] = gt_v + gen.normal(0, 0.02, (B, 12, 3))
    offset = lambda i: i * (2 * V - i - 1) // 2                              # noqa: E731
    label_e = np.array([offset(i) + j - i - 1 for i, j in gt_e])
    probs = gen.uniform(0.0, 0.45, (B, max_e)).astype(np.float32)
    for s in range(B):
        probs[s, gen.choice(max_e, (3 * V) // 2 - len(label_e), replace=False)] = 0.8
        probs[s, label_e] = 0.9
    return {"vertices": torch.from_numpy(verts).to(dev)[:, :, :3], "edge_probs": torch.from_numpy(probs).to(dev),
            "counts": torch.full((B,), V, dtype=torch.int64, device=dev), "kept": int((probs > 0.5).sum()),
            "labels": ([torch.from_numpy(gt_v)] * B, [torch.from_numpy(gt_e.astype(np.float32))] * B)}


def predictions(data, V, layout):
    pred = {"vertices": data["vertices"], "edge_probs": data["edge_probs"]}
    if layout == "padded":
        pred["edge_counts"] = data["counts"]
        pred["edge_indices"] = EdgeIndexLists(data["counts"])
    else:
        pred["edge_indices"] = edge_index_lists([V] * B)
    return pred


def blocks_of(arms, blocks, steps, warmup):
    """{arm: block medians} of the per-call milliseconds, in alternating blocks"""
    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3
    for fn in arms.values():
        for _ in range(warmup):
            fn()
    med = {k: [] for k in arms}
    for _ in range(blocks):
        for name, fn in arms.items():
            med[name].append(float(np.median([timed(fn) for _ in range(steps)])))
    return med


def summary(v, digits=3):
    return {"median": round(float(np.median(v)), digits), "block_spread": round(max(v) - min(v), digits)}


def same_wireframes(a, b):
    return all(x[k].dtype == y[k].dtype and x[k].shape == y[k].shape and np.array_equal(x[k], y[k])
               for x, y in zip(a, b) for k in ("pred_vertices", "pd_edges", "pd_edges_vertices"))


def run(V, layout, data, args):
    max_e, K = V * (V - 1) // 2, data["kept"]
    pred = lambda: predictions(data, V, layout)                              # noqa: E731

    def evaluate(compact):
        calc = ap.APCalculator(distance_thresh=0.1)
        postprocess.evaluate_batch(pred(), *data["labels"], calc, compact=compact)
        return calc

    pairs = {"wireframes": (lambda: postprocess.wireframes_from_predictions(pred()), lambda: postprocess.wireframes_compact(pred())),
             "evaluate": (lambda: evaluate(False), lambda: evaluate(True))}
    same = {"wireframes": same_wireframes(pairs["wireframes"][0](), pairs["wireframes"][1]())}
    c_old, c_new = evaluate(False), evaluate(True)
    same["evaluate"] = all(float(c_old.ap_dict[k]) == float(c_new.ap_dict[k]) for k in c_old.ap_dict)
    nbytes = {"old": B * (3 * V + 7 * max_e) * 4, "compact": (B + 1) * 4 + 12 * B * V + 36 * K}
    lines = []
    for what, (old, new) in pairs.items():
        med = blocks_of({"old": old, "compact": new}, args.blocks, args.block_steps, args.warmup)
        o, n = summary(med["old"]), summary(med["compact"])
        common = {"bench": "evalpost", "what": what, "B": B, "V": V, "max_e": max_e, "layout": layout, "kept_edges": K,
                  "blocks": args.blocks, "steps_per_block": args.block_steps}
        lines.append(dict(common, arm="old", ms=o, d2h_bytes=nbytes["old"]))
        lines.append(dict(common, arm="compact", ms=n, d2h_bytes=nbytes["compact"], same_results=same[what],
                          old_over_compact=round(o["median"] / n["median"], 2),
                          faster_by_more_than_old_spread=bool(o["median"] - n["median"] > o["block_spread"])))
    return lines


def worst_case(gen, dev):
    """V = 64, every candidate kept, a 300-edge label on 120 random vertices"""
    V, max_e = 64, 2016
    gt_v = gen.uniform(-8, 8, (120, 3)).astype(np.float32)
    every = np.stack(np.triu_indices(120, 1), axis=1)
    gt_e = every[np.sort(gen.choice(len(every), 300, replace=False))].astype(np.int64)
    verts = gen.uniform(-8, 8, (B, V, 4)).astype(np.float32)
    verts[:, :, :3] = gt_v[:V] + gen.normal(0, 0.02, (B, V, 3))
    return {"vertices": torch.from_numpy(verts).to(dev)[:, :, :3], "edge_probs": torch.full((B, max_e), 0.9, device=dev),
            "counts": torch.full((B,), V, dtype=torch.int64, device=dev), "kept": B * max_e,
            "labels": ([torch.from_numpy(gt_v)] * B, [torch.from_numpy(gt_e.astype(np.float32))] * B)}


def run_metrics(V, layout, data, args, thresh, blocks, steps, warmup, tag=None):
    pred = lambda: predictions(data, V, layout)                              # noqa: E731
    labels = postprocess.EvalLabels(*data["labels"], data["vertices"].device)

    def evaluate(metrics, lab=None):
        calc = ap.APCalculator(distance_thresh=thresh)
        postprocess.evaluate_batch(pred(), *data["labels"], calc, compact=True, metrics=metrics, labels=lab)
        return calc

    arms = {"compact": lambda: evaluate("host"), "device": lambda: evaluate("device"),
            "device_labels": lambda: evaluate("device", labels)}
    ref = arms["compact"]()
    same = {}
    for name in ("device", "device_labels"):
        got = arms[name]()
        same[name] = all(int(ref.ap_dict[k]) == int(got.ap_dict[k]) for k in ("tp_corners", "tp_fp_corners", "tp_fn_corners",
                                                                                "tp_edges", "tp_fp_edges", "tp_fn_edges")) and \
            all(np.isclose(float(ref.ap_dict[k]), float(got.ap_dict[k]), rtol=1e-12, atol=0.0) for k in ("distance", "wed"))
    med = blocks_of(arms, blocks, steps, warmup)
    c = summary(med["compact"])
    common = {"bench": "evalmetrics", "what": tag or "evaluate", "B": B, "V": V, "max_e": V * (V - 1) // 2, "layout": layout,
              "kept_edges": data["kept"], "label_edges": int(len(data["labels"][1][0])), "blocks": blocks, "steps_per_block": steps}
    lines = [dict(common, arm="compact", ms=c)]
    for name in ("device", "device_labels"):
        n = summary(med[name])
        lines.append(dict(common, arm=name, ms=n, same_results=same[name], compact_over_device=round(c["median"] / n["median"], 2),
                          ahead_by_more_than_the_larger_spread=bool(c["median"] - n["median"] > max(c["block_spread"], n["block_spread"]))))
    return lines


def run_decode(V, data, args):
    pred = lambda ex: dict(predictions(data, V, "padded"), existence_probabilities=ex)      # noqa: E731
    labels = postprocess.EvalLabels(*data["labels"], data["vertices"].device)
    gen = np.random.RandomState(1)
    alive = gen.uniform(0.6, 0.99, (B, V)).astype(np.float32)
    sparse = np.where(gen.uniform(0, 1, (B, V)) < 0.25, alive, np.float32(0.1))
    sparse[:, :12] = alive[:, :12]
    ex = {"decoded": torch.from_numpy(alive).to(data["vertices"].device), "decoded_sparse": torch.from_numpy(sparse).to(data["vertices"].device)}
    opts = {"existence_threshold": 0.5, "merge_radius": 0.05}

    def evaluate(arm):
        calc = ap.APCalculator(distance_thresh=0.1)
        postprocess.evaluate_batch(pred(ex.get(arm, ex["decoded"])), *data["labels"], calc, compact=True, metrics="device",
                                   labels=labels, decode=None if arm == "undecoded" else opts)
        return calc

    arms = {name: (lambda name=name: evaluate(name)) for name in ("undecoded", "decoded", "decoded_sparse")}
    ref = {name: fn() for name, fn in arms.items()}
    med = blocks_of(arms, args.blocks, args.block_steps, args.warmup)
    u = summary(med["undecoded"])
    common = {"bench": "decode", "what": "evaluate", "B": B, "V": V, "max_e": V * (V - 1) // 2, "layout": "padded",
              "kept_edges": data["kept"], "blocks": args.blocks, "steps_per_block": args.block_steps}
    lines = []
    for name in arms:
        m = summary(med[name])
        lines.append(dict(common, arm=name, ms=m, decoded_minus_undecoded_ms=round(m["median"] - u["median"], 3),
                          tp_fp_corners=int(ref[name].ap_dict["tp_fp_corners"]), tp_fp_edges=int(ref[name].ap_dict["tp_fp_edges"]),
                          tp_edges=int(ref[name].ap_dict["tp_edges"])))
    return lines


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--blocks", type=int, default=5)
    p.add_argument("--block-steps", type=int, default=7)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--vertices", default="64,256")
    p.add_argument("--what", choices=("compact", "metrics", "decode"), default="compact")
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", {"compact": "r13_evalpost.jsonl", "metrics": "r15_evalmetrics.jsonl",
                                                   "decode": "r20_decode.jsonl"}[args.what])
    dev = torch.device("cuda:0")
    ap.set_device(dev)
    gen = np.random.RandomState(0)

    def emit(lines):
        for r in lines:
            print(json.dumps(r), flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(json.dumps(r) + "\n")

    for V in (int(v) for v in args.vertices.split(",")):
        data = synthetic(V, gen, dev)
        if args.what == "decode":
            emit(run_decode(V, data, args))
            continue
        for layout in ("ragged", "padded"):
            if args.what == "compact":
                emit(run(V, layout, data, args))
            else:
                emit(run_metrics(V, layout, data, args, 0.1, args.blocks, args.block_steps, args.warmup))
    if args.what == "metrics":
        emit(run_metrics(64, "padded", worst_case(gen, dev), args, 0.1, 3, 2, 1, tag="worst_case_all_kept"))


if __name__ == "__main__":
    main()
