"""GPU time of one wf3d.meter.WireframeMeter.update (two launches, csrc/metrics.hip) at the cfg2 and cfg5 loss shapes
(B=32, V=64 and V=256, counts U{4..V}), with wf3d_meter_update (TrainMeter.update) and the pieces of the device loss
measured in the same process as yardsticks.  Device events around one eager call, median of --reps after warm-up; the
`_replayed` figures are a captured graph of 20 calls over 20: the device side without the eager call's host time.
Prints one JSON line per shape."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "wireframe-3d-prediction_amd"))
import torch  # noqa: E402
from wf3d import ops  # noqa: E402
from wf3d.meter import TrainMeter, WireframeMeter  # noqa: E402
from losses.WireframeLoss import WireframeLoss  # noqa: E402


def timeit(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(ts)


def replayed(fn, reps, n=20):
    """us per call inside a captured graph of n calls: the device side without the eager call's host time."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(n):
            fn()
    return timeit(graph.replay, max(reps // 4, 10)) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vs", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_meter.py needs a GPU"
    dev = torch.device("cuda:0")
    for V in a.vs:
        B, E = a.batch, V * (V - 1) // 2
        torch.manual_seed(0)
        counts = torch.randint(4, V + 1, (B,), device=dev)
        pred = {"vertices": torch.randn(B, V, 4, device=dev)[:, :, :3], "existence_probabilities": torch.rand(B, V, device=dev),
                "edge_probs": torch.rand(B, E, device=dev)}
        tgt = {"vertices": torch.randn(B, V, 3, device=dev),
               "vertex_existence": (torch.arange(V, device=dev)[None] < counts[:, None]).float(),
               "edge_labels": (torch.rand(B, E, device=dev) > 0.8).float(), "vertex_counts": counts}
        crit = WireframeLoss(3.0, 1.5, 1.0)
        res = crit(pred, tgt)
        c4r = crit.last_assignment
        qm, tm = WireframeMeter(dev), TrainMeter(dev)
        pe = pred["existence_probabilities"]
        cost = ops.loss_cost_matrix(pred["vertices"], pe, tgt["vertices"], counts)
        def update():
            qm.update(pred, tgt, c4r)

        def train_meter():
            tm.update(res, pred["vertices"], tgt["vertices"], counts)

        def terms():
            ops.loss_terms_assigned(pred["vertices"], pe, pred["edge_probs"], tgt["vertices"], tgt["vertex_existence"],
                                    tgt["edge_labels"], c4r, counts, (3.0, 1.0, 1.5))
        us = {
            "wireframe_meter_update": timeit(update, a.reps),
            "train_meter_update": timeit(train_meter, a.reps),
            "loss_terms": timeit(terms, a.reps),
            "loss_assign": timeit(lambda: ops.loss_assign(cost), a.reps),
            "loss_forward": timeit(lambda: crit(pred, tgt), a.reps),
            "wireframe_meter_update_replayed": replayed(update, a.reps),
            "train_meter_update_replayed": replayed(train_meter, a.reps),
            "loss_terms_replayed": replayed(terms, a.reps),
        }
        read_bytes = 2 * B * E * 4 + B * V * (12 + 12 + 4 + 4 + 4)
        print(json.dumps({"B": B, "V": V, "E": E, "us": {k: round(v, 2) for k, v in us.items()}, "update_read_bytes": read_bytes,
                          "update_over_loss_forward": round(us["wireframe_meter_update"] / us["loss_forward"], 4),
                          "update_over_loss_terms": round(us["wireframe_meter_update"] / us["loss_terms"], 4),
                          "replayed_update_over_loss_terms": round(us["wireframe_meter_update_replayed"] / us["loss_terms_replayed"], 4)}),
              flush=True)


if __name__ == "__main__":
    main()
