"""The fp64 oracle over a batch too large to hold at once, a few samples at a time (TEST INFRASTRUCTURE, like the rest of
oracle/: used by tests/test_bench_configs_gpu.py).

No operation of the model mixes samples: the encoder's per-point MLP works on rows, its pools and both heads on one
cloud each, the edge head on one sample's vertices (tests/test_dp_gpu.py relies on the same fact).
So the outputs of oracle.reference_cpu.model_forward over samples [s0, s1) are those rows of the whole batch's outputs,
and the parameter gradient of sum_k <out_k, cot_k> is the sum over chunks of each chunk's.  Running the oracle chunk by
chunk is exact, not an approximation; what it saves is memory (at B = 32, N = 4096, V = 256 the whole batch's fp64
activations and dropout masks would take tens of GB).  The arithmetic is reference_cpu's, on whatever device the
parameters and inputs are on."""
import torch

from . import reference_cpu as oracle

COT_KEYS = ("vertices", "existence_probabilities", "edge_probs")


def slice_frozen(frozen, s0, s1, n_points):
    """The decisions of samples [s0, s1) out of a batch's frozen dict (oracle.frozen.capture_decisions): the per-point
    encoder masks by rows s0 * N .. s1 * N, the head masks and the pools' arg-max rows by sample."""
    if frozen is None:
        return None
    relu = {k: (m[s0 * n_points:s1 * n_points] if k.startswith("encoder.mlp.") else m[s0:s1])
            for k, m in frozen.get("relu", {}).items()}
    argmax = {k: a[s0:s1] for k, a in frozen.get("argmax", {}).items()}
    return {"relu": relu, "argmax": argmax}


def model_forward_chunked(P, x, target_vertex_counts, max_vertices, chunk, cot=None, frozen=None, drop=None,
                          training=True, num_heads=8):
    """oracle.reference_cpu.model_forward over samples [s, s + chunk) at a time.

    cot: {key: cotangent} for COT_KEYS (edge_probs as wide as the batch's padded output); when given, each chunk's
    sum_k <out_k, cot_k> is back-propagated, so P's .grad hold the whole batch's gradient at the end.  Without it the
    forward runs under no_grad.
    frozen: the whole batch's decisions (sliced per chunk here).
    drop: callable (s0, s1) -> per-sample edge-head masks of samples [s0, s1) (oracle.dropout.edge_head_masks with
    s0, s1), built per chunk so that only one chunk's masks exist at a time; None is no dropout.

    Returns the outputs as model_forward does, detached: tensors concatenated over the batch, edge_probs zero-padded to
    the batch's widest sample, edge_indices one list per sample."""
    B, N = x.shape[0], x.shape[1]
    parts = {k: [] for k in ("vertices", "existence_probabilities", "global_features", "actual_vertex_counts")}
    probs, indices = [], []
    for s0 in range(0, B, chunk):
        s1 = min(B, s0 + chunk)
        counts = None if target_vertex_counts is None else target_vertex_counts[s0:s1]
        with torch.set_grad_enabled(cot is not None):
            ref = oracle.model_forward(P, x[s0:s1], counts, max_vertices, training=training, num_heads=num_heads,
                                       frozen=slice_frozen(frozen, s0, s1, N),
                                       drop=None if drop is None else drop(s0, s1))
            if cot is not None:
                w = ref["edge_probs"].shape[1]
                loss = sum((ref[k] * cot[k][s0:s1, :w].to(ref[k]) if k == "edge_probs" else
                            ref[k] * cot[k][s0:s1].to(ref[k])).sum() for k in COT_KEYS)
                loss.backward()
        for k in parts:
            parts[k].append(ref[k].detach())
        probs.append(ref["edge_probs"].detach())
        indices.extend(ref["edge_indices"])
        del ref
    out = {k: torch.cat(v) for k, v in parts.items()}
    width = max(p.shape[1] for p in probs)
    out["edge_probs"] = torch.cat([torch.nn.functional.pad(p, (0, width - p.shape[1])) for p in probs])
    out["edge_indices"] = indices
    return out
