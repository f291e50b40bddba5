"""Forward-only (eval, no_grad) time and memory of the drop-in model — the evaluate.py:71 call — on the training forward
("train") and on the forward-only stream path (wf3d.infer, "stream"), alternated inside one process.

  python scripts/bench_inference.py --shape cfg2 --rows 4096,8192,16384,32768,M [--path both] [--precision bf16x3]

--shape  cfg2 (B=32, N=4096), cfg4 (B=8, N=16384), tile (B=1, N=1048576: one LiDAR tile, what the stream path is for)
--path   train | stream | both.  "train" is timed twice (train, train-again): the difference of the two medians is the
         run-to-run spread that a difference between the paths has to beat.
--rows   block heights of the stream path, comma separated; M = all rows in one block.
Every configuration is warmed up, then --iters (>= 20) forwards of each are timed with device events, round robin, so
that clocks and cache state are shared between the paths.  Peak allocated bytes are those of one more forward per
configuration, over what was allocated before it.  One JSON line per configuration (also appended to --out).

Edge-head mode: the shapes edge-cfg2 (B=32, V=64: 64,512 edge rows), edge-cfg5 (B=32, V=256: 1,044,480) and
edge-cfg5-padded run EdgePredictor alone, eval(), no_grad, on EdgeFn ("train") and on wf3d.infer.edge_stream ("stream",
--rows = its block heights, M = all edge rows).  The first two take forward_ragged with counts = V; the padded one takes
forward_padded(tail="skip") with device counts drawn from U{4..38}, the data set's range, at max_vertices = 256.

  python scripts/bench_inference.py --shape edge-cfg5 --rows 8192,16384,32768,65536,131072"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "wireframe-3d-prediction_amd"))
import torch  # noqa: E402

from models.EdgePredictor import EdgePredictor  # noqa: E402
from models.PointCloudToWireframe import PointCloudToWireframe  # noqa: E402
from wf3d import config  # noqa: E402

SHAPES = {"cfg2": (32, 4096, 64), "cfg4": (8, 16384, 64), "tile": (1, 1 << 20, 64)}
EDGE_SHAPES = {"edge-cfg2": (32, 64, False), "edge-cfg5": (32, 256, False), "edge-cfg5-padded": (32, 256, True)}   # B, V, padded


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="cfg2", choices=sorted(SHAPES) + sorted(EDGE_SHAPES))
    ap.add_argument("--path", default="both", choices=["train", "stream", "both"])
    ap.add_argument("--rows", default=None, help="default: config.INFER_ROWS, or config.INFER_EDGE_ROWS for an edge shape")
    ap.add_argument("--precision", default=config.precision(), choices=config.PRECISIONS)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.iters < 20:
        ap.error("--iters must be at least 20")
    config.set_precision(a.precision)
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    edge = a.shape in EDGE_SHAPES
    if edge:
        B, V, padded = EDGE_SHAPES[a.shape]
        N, M = None, B * (V * (V - 1) // 2)        # the rows the stream path walks: edge rows
        head = EdgePredictor().to(dev).eval()
        verts = torch.randn(B, V, 3, device=dev)
        counts = torch.randint(4, 39, (B,), generator=torch.Generator().manual_seed(1)).to(dev) if padded else [V] * B
        extra = {"edge_rows": M, "layout": "padded/skip" if padded else "ragged"}
        if padded:
            extra["live_edge_rows"] = int((counts * (counts - 1) // 2).sum())
    else:
        B, N, V = SHAPES[a.shape]
        M = B * N
        model = PointCloudToWireframe(input_dim=8, max_vertices=V).to(dev).eval()
        with torch.no_grad():                          # make the untrained model predict >= 2 vertices per sample
            model.vertex_predictor.final_layer.bias.view(V, 4)[:, 3].fill_(3.0)
        x = torch.randn(B, N, 8, device=dev)
        extra = {}
    if a.rows is None:
        a.rows = str(config.INFER_EDGE_ROWS if edge else config.INFER_ROWS)

    cfgs = []                                      # (label, path, rows)
    if a.path in ("train", "both"):
        cfgs += [("train", "train", None), ("train-again", "train", None)]
    if a.path in ("stream", "both"):
        for r in a.rows.split(","):
            rows = M if r.strip() == "M" else int(r)
            cfgs.append((f"stream-{rows}", "stream", rows))

    def forward(path, rows):
        with torch.no_grad():
            if edge:
                config.set_edge_inference(path)
                if rows is not None:
                    config.INFER_EDGE_ROWS = rows
                return head.forward_padded(verts, counts, tail="skip") if padded else head.forward_ragged(verts, counts)
            config.set_inference(path)
            if rows is not None:
                config.INFER_ROWS = rows
            return model(x)

    times = {c[0]: [] for c in cfgs}
    for label, path, rows in cfgs:
        for _ in range(a.warmup):
            forward(path, rows)
    torch.cuda.synchronize()
    for _ in range(a.iters):
        for label, path, rows in cfgs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            forward(path, rows)
            e1.record()
            torch.cuda.synchronize()
            times[label].append(e0.elapsed_time(e1))
    peaks = {}
    for label, path, rows in cfgs:
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = forward(path, rows)
        torch.cuda.synchronize()
        peaks[label] = torch.cuda.max_memory_allocated() - before
        del out
    config.set_inference("train")
    config.set_edge_inference("train")
    lines = []
    for label, path, rows in cfgs:
        t = statistics.median(times[label])
        lines.append(json.dumps({"shape": a.shape, "B": B, "N": N, "V": V, "precision": a.precision, "config": label,
                                 "path": path, "rows": rows, "iters": a.iters, "median_ms": round(t, 4),
                                 "min_ms": round(min(times[label]), 4), "max_ms": round(max(times[label]), 4),
                                 "clouds_per_s": round(B / t * 1e3, 1), "peak_bytes": int(peaks[label]), **extra}))
    for ln in lines:
        print(ln, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
