"""wf3d_edge_labels_matched (csrc/loss.hip) against its specification wf3d.targets.matched_edge_labels: equal element for
element.  Shapes: no pairs at all, the smallest pair, counts 0 and above V (clamped), pair counts d_b on both sides of
the target counts c_b, labels narrower than the pair order needs, an output wider than any d_b(d_b-1)/2, B > 64, more
than one 256-wide trip of the staging loop and more than one column chunk, and the limit V = 1024.  Assignment rows:
random permutations, scipy-style rows with V in the unmatched slots, rows with negative entries, rows with a repeated
entry.  One test hands the entry a NaN-filled buffer: every element is written, and nothing past the last row."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (B, V, Vt, Et, Ep); Et / Ep None: the full width of Vt / V vertices
SHAPES = {
    "no_pairs": (1, 1, 1, 0, 0),
    "one_pair": (2, 2, 2, None, None),
    "clamped_counts": (3, 9, 5, None, None),
    "narrow_labels": (4, 12, 12, 30, None),
    "wide_output": (3, 6, 6, None, 40),
    "B70": (70, 5, 5, None, None),
    "V320": (2, 320, 320, None, None),
    "V1024": (1, 1024, 1024, None, None),
}


def dev():
    return torch.device("cuda:0")


def full(v):
    return v * (v - 1) // 2


def build(name, pair_mode):
    B, V, Vt, Et, Ep = SHAPES[name]
    Et, Ep = full(Vt) if Et is None else Et, full(V) if Ep is None else Ep
    rng = np.random.default_rng(sum(map(ord, name)) * 7 + len(pair_mode))
    tl = (rng.random((B, Et)) > 0.6).astype(np.float32)
    top = min(V, Vt)
    counts = rng.integers(0, top + 1, B)
    counts[0] = top
    if name == "clamped_counts":
        counts[:] = (0, V + 4, 5)            # the kernel clamps to 0..V; the label row is narrower than 9 vertices need
    a = np.stack([rng.permutation(V) for _ in range(B)]).astype(np.int32)
    for b in range(B):
        kind = b % 4                         # 0: permutation
        if kind == 1:
            a[b][a[b] >= counts[b]] = V      # scipy-style: V in the unmatched slots
        elif kind == 2 and V > 1:
            a[b, rng.integers(0, V, max(1, V // 4))] = -1 - rng.integers(0, 5)
        elif kind == 3 and V > 1:
            i, j = rng.choice(V, 2, replace=False)
            a[b, i] = a[b, j]                # a repeated entry: the pair (i, j) has tp == tq
    if B == 1 and V > 1:                     # one row: give it a bit of everything
        a[0, 3 % V] = V
        a[0, 5 % V] = -2
        a[0, 1] = a[0, 0]
    pair = {"none": None, "below": np.maximum(counts - 2, 0), "above": np.minimum(counts + 3, V + 2),
            "random": rng.integers(-1, V + 3, B)}[pair_mode]
    return tl, a, counts, Ep, pair


# d_b = c_b, d_b < c_b, d_b > c_b, and any value including ones the kernel clamps; the two largest shapes take two of them
CASES = [(n, m) for n in SHAPES for m in ("none", "below", "above", "random")
         if n not in ("V1024", "B70") or m in ("none", "random")]


@pytest.mark.parametrize("name, pair_mode", CASES, ids=[f"{n}-{m}" for n, m in CASES])
def test_kernel_equals_the_spec(name, pair_mode):
    from wf3d import ops
    from wf3d.targets import matched_edge_labels
    tl, a, counts, Ep, pair = build(name, pair_mode)
    want = matched_edge_labels(tl, a, counts, Ep, pair)
    t = lambda x, dt: None if x is None else torch.as_tensor(np.asarray(x), dtype=dt).to(dev())     # noqa: E731
    got = ops.edge_labels_matched(t(tl, torch.float32), t(a, torch.int32), t(counts, torch.int64), Ep, t(pair, torch.int64))
    assert got.shape == want.shape and got.dtype == torch.float32
    got = got.cpu().numpy()
    print(f"{name}/{pair_mode}: {want.shape}, ones {int(want.sum())}, differing {int((got != want).sum())}")
    assert np.array_equal(got, want)
    if pair_mode == "none" and name not in ("no_pairs", "one_pair"):
        assert want.sum() > 0                # the case says something


def test_every_element_is_written():
    """The entry writes into the caller's buffer: a NaN-filled one comes back without a NaN, dead columns included."""
    from wf3d import _lib, ops
    from wf3d.targets import matched_edge_labels
    tl, a, counts, Ep, pair = build("wide_output", "above")
    B, V = a.shape
    d = lambda x, dt: torch.as_tensor(np.asarray(x), dtype=dt).to(dev())     # noqa: E731
    tl_d, a_d, c_d, p_d = d(tl, torch.float32), d(a, torch.int32), d(counts, torch.int64), d(pair, torch.int64)
    out = torch.full((B, Ep + 3), float("nan"), device=dev())               # three guard columns behind the last row
    flat = out.view(-1)[:B * Ep]
    _lib.check(_lib.load().wf3d_edge_labels_matched(tl_d.data_ptr(), tl.shape[1], a_d.data_ptr(), c_d.data_ptr(), p_d.data_ptr(),
                                                    B, V, Ep, flat.data_ptr(), ops._stream()), "edge_labels_matched")
    torch.cuda.synchronize()
    assert np.array_equal(flat.cpu().numpy().reshape(B, Ep), matched_edge_labels(tl, a, counts, Ep, pair))
    assert bool(torch.isnan(out.view(-1)[B * Ep:]).all())                   # and nothing past it


def test_wrapper_rejects_bad_inputs():
    from wf3d import ops
    tl = torch.zeros(2, 6, device=dev())
    a = torch.zeros(2, 4, dtype=torch.int32, device=dev())
    c = torch.zeros(2, dtype=torch.int64, device=dev())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.edge_labels_matched(tl.cpu(), a, c, 6)
    with pytest.raises(RuntimeError, match="bad layout / dtype"):
        ops.edge_labels_matched(tl, a.long(), c, 6)
    with pytest.raises(RuntimeError, match="batch sizes differ"):
        ops.edge_labels_matched(tl, a, c[:1], 6)
    assert ops.edge_labels_matched(tl, a, c, 0).shape == (2, 0)
