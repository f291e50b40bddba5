"""Packed point-cloud batches, the parts that need no GPU: the fixture tests/golden/packed.npz (the reference model on each
cloud alone, B = 1) against the CPU oracle, the host side of the row layout, pack / collate_packed, and the C ABI."""
import numpy as np
import pytest
import torch

import helpers as H
from helpers import detgen, oracle

TOL = 2e-6          # tests/test_oracle_golden.py
KEYS = ("vertices", "existence_probabilities", "edge_probs")


def packed_case():
    """(gold, clouds [1, N_b, 8] float32 arrays, state_dict arrays, vertex counts, V, seed) of packed.npz."""
    gold = H.load_golden("packed")
    seed, V = int(gold["meta.seed"]), int(gold["meta.V"])
    tb, tn = (int(v) for v in gold["meta.zero_tail"])
    clouds = []
    for b, n in enumerate(int(v) for v in gold["meta.point_counts"]):
        x = detgen.normalish(f"packed.x{b}", (1, n, 8), seed)
        if b == tb:
            x[0, n - tn:] = 0.0
        clouds.append(x)
    arrs = detgen.fill_state_dict(oracle.state_dict_shapes(8, V), seed)
    return gold, clouds, arrs, [int(c) for c in gold["meta.counts"]], V, seed


def packed_cotangents(b, out, seed):
    return {k: torch.from_numpy(detgen.uniform(f"packed.cot{b}.{k}", tuple(out[k].shape), -1, 1, seed)) for k in KEYS}


def test_fixture_has_the_cases_the_feature_is_about():
    gold = H.load_golden("packed")
    pc = gold["meta.point_counts"].tolist()
    assert len(pc) == 4 and len(set(pc)) == 4 and min(pc) < 64
    assert int(gold["meta.zero_tail"][1]) > 0
    assert not any(k.endswith(".weight") or k.endswith(".bias") for k in gold)       # results and recipes only


def test_oracle_per_cloud_reproduces_packed_fixture():
    gold, clouds, arrs, counts, V, seed = packed_case()
    P = oracle.params_from_numpy(arrs)
    loss_sum, lens, flat = 0.0, [], []
    for b, x in enumerate(clouds):
        out = oracle.model_forward(P, torch.from_numpy(x), torch.tensor(counts[b:b + 1]), V, training=True)
        for k in ("vertices", "existence_probabilities", "global_features"):
            assert H.rel_err(out[k].detach().numpy()[0], gold["out." + k][b]) < TOL, (b, k)
        e = out["edge_probs"].shape[1]
        assert H.rel_err(out["edge_probs"].detach().numpy()[0], gold["out.edge_probs"][b, :e]) < TOL, b
        assert np.all(gold["out.edge_probs"][b, e:] == 0.0)
        assert int(out["actual_vertex_counts"][0]) == int(gold["out.actual_vertex_counts"][b])
        lens.append(len(out["edge_indices"][0]))
        flat += list(out["edge_indices"][0])
        cot = packed_cotangents(b, out, seed)
        loss = sum((out[k] * cot[k]).sum() for k in cot)
        loss.backward()                           # accumulates: the sum over the clouds
        loss_sum += loss.item()
    assert lens == gold["out.edge_index_lens"].tolist()
    assert np.array_equal(np.array(flat, dtype=np.int64).reshape(-1, 2), gold["out.edge_indices_flat"])
    assert abs(loss_sum - float(gold["out.loss"])) < 1e-5 * max(1.0, abs(float(gold["out.loss"])))
    bad = H.check_grad_summaries(gold, [(n, p.grad) for n, p in P.items()], 1e-5)
    assert not bad, bad


@pytest.mark.parametrize("counts", [[1], [1, 5, 300, 4097], [256], [700, 1300, 2096, 517], [4096] * 32, [14039, 1276, 64]])
def test_layout_offsets_padding_row_map_and_chunks(counts):
    from wf3d.ops import PackedLayout, ROW_PAD
    lay = PackedLayout(counts)
    M = sum(counts)
    assert ROW_PAD == 256
    assert lay.B == len(counts) and lay.M == M
    assert lay.offsets.tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist()
    assert lay.M_pad % 256 == 0 and 0 <= lay.M_pad - M < 256
    rm = lay.row_map()
    assert rm.shape == (lay.M_pad,) and np.all(rm[M:] == -1)
    for b in range(lay.B):
        assert np.all(rm[lay.offsets[b]:lay.offsets[b + 1]] == b)
    # the clouds' chunks tile rows 0 .. M-1 in order, never cross a cloud, and are at most chunk_rows long
    ck = lay.chunks
    assert ck.shape == (lay.nchunk_bwd, 4) and lay.nchunk_bwd == lay.nchunk + (lay.M_pad > M)
    row = 0
    for k in range(lay.nchunk):
        b, first, r0, r1 = ck[k].tolist()
        assert first == lay.offsets[b] and r0 == row and r0 < r1 <= lay.offsets[b + 1] and r1 - r0 <= lay.chunk_rows
        assert lay.chunk_offsets[b] <= k < lay.chunk_offsets[b + 1]
        row = r1
    assert row == M and lay.chunk_offsets[-1] == lay.nchunk
    if lay.M_pad > M:
        assert ck[-1].tolist() == [-1, 0, M, lay.M_pad]
    assert lay.nchunk <= 256 + lay.B                         # fills the chip whatever the counts, no more


def test_layout_equal_lengths_matches_the_dense_split():
    """[4096] * 32 (cfg2): 512-row chunks, eight per cloud — the split the dense pool takes at that shape."""
    from wf3d.ops import PackedLayout
    lay = PackedLayout([4096] * 32)
    assert lay.M_pad == lay.M == 131072 and lay.chunk_rows == 512 and lay.nchunk == lay.nchunk_bwd == 256


@pytest.mark.parametrize("bad", [[], [3, 0, 2], [4, -1]])
def test_layout_rejects_bad_counts(bad):
    from wf3d.ops import PackedLayout
    with pytest.raises(ValueError):
        PackedLayout(bad)


def test_point_counts_accept_cpu_tensors_only_as_ints():
    from wf3d.ops import point_counts_list
    assert point_counts_list(torch.tensor([3, 4])) == [3, 4]
    assert point_counts_list((5,)) == [5]
    with pytest.raises(ValueError):
        point_counts_list(torch.tensor([3.0, 4.0]))
    with pytest.raises(ValueError):
        point_counts_list(torch.tensor([[3, 4]]))


def test_pack():
    from wf3d.packed import pack
    a, b = torch.randn(5, 8), np.ones((3, 8), dtype=np.float64)
    pts, counts = pack([a, b])
    assert counts == [5, 3] and pts.shape == (8, 8) and pts.dtype == torch.float32 and pts.is_contiguous()
    assert torch.equal(pts[:5], a) and torch.all(pts[5:] == 1.0)
    for bad in ([], [torch.randn(5, 8), torch.randn(3, 6)], [torch.randn(0, 8)], [torch.randn(8)]):
        with pytest.raises(ValueError):
            pack(bad)


def test_collate_packed():
    from datasets.building3d import Building3DReconstructionDataset as DS
    rng = np.random.default_rng(0)
    items = []
    for i, n in enumerate((7, 3, 11)):
        items.append({"point_clouds": rng.standard_normal((n, 8)).astype(np.float32),
                      "wf_vertices": rng.standard_normal((4 + i, 3)), "wf_edges": np.array([[0, 1], [1, 2]]),
                      "wf_centers": rng.standard_normal((2, 3)), "wf_edges_vertices": rng.standard_normal((2, 6)),
                      "centroid": rng.standard_normal(3), "max_distance": float(i + 1), "scan_idx": i})
    out = DS.collate_packed(items)
    assert out["point_counts"].tolist() == [7, 3, 11] and out["point_counts"].dtype == torch.int64
    assert out["point_clouds"].shape == (21, 8) and out["point_clouds"].is_contiguous()
    assert np.array_equal(out["point_clouds"][7:10].numpy(), items[1]["point_clouds"])
    ref = DS.collate_batch([{k: v for k, v in it.items() if k != "point_clouds"} for it in items])
    assert set(out) == set(ref) | {"point_clouds", "point_counts"}
    for k, v in ref.items():
        if isinstance(v, list):
            assert all(torch.equal(a, b) for a, b in zip(out[k], v)), k
        else:
            assert torch.equal(out[k], v), k
    with pytest.raises(ValueError):
        DS.collate_packed([])


SEG = ("wf3d_pool4_seg_ws_bytes", "wf3d_pool4_seg_fwd", "wf3d_pool4_seg_bwd", "wf3d_pool4_seg_bwd_sx8")


def test_library_exports_the_segmented_pool():
    from wf3d import _lib
    lib = _lib.load()
    for n in SEG:
        assert hasattr(lib, n), n
    assert lib.wf3d_pool4_seg_ws_bytes(256, 512) >= 256 * 512 * 24 + 256 * 4
    assert lib.wf3d_pool4_seg_ws_bytes(0, 512) == 0
    # argument checks are reachable without a GPU
    assert lib.wf3d_pool4_seg_fwd(None, None, None, None, None, 2, 1, 2, 64, None, None, None, None, 128, None, None, None, None,
                                  None, 0, None) == -1
    assert b"bad dims" in lib.wf3d_last_error()
    assert lib.wf3d_pool4_seg_bwd(None, None, None, None, None, None, 0, None, None, 0, None, None, None, 2, 8, 256, 3, 256, 64,
                                  None, None) == -1
    assert b"null pointer" in lib.wf3d_last_error()


def test_bindings_and_host_functions_exist():
    from wf3d import _lib, ops
    from models.PointCloudToWireframe import PointCloudToWireframe
    from models.PointNetEncoder import PointNetEncoder
    from wf3d.functional import EncoderFnPacked
    for n in SEG:
        assert n in _lib.SIGNATURES, n
    for f in ("pool4_seg_fwd", "pool4_seg_bwd", "pool4_seg_bwd_colsum", "PackedLayout"):
        assert hasattr(ops, f), f
    assert hasattr(PointNetEncoder, "encode_packed") and hasattr(PointCloudToWireframe, "forward_packed")
    assert EncoderFnPacked.__name__.startswith("EncoderFn")


def test_forward_packed_host_errors_need_no_gpu():
    from models.PointCloudToWireframe import PointCloudToWireframe
    m = PointCloudToWireframe(8, 4)
    x = torch.zeros(10, 8)
    with pytest.raises(ValueError, match="sum to"):
        m.forward_packed(x, [4, 5])
    with pytest.raises(ValueError, match="at least one point"):
        m.forward_packed(x, [10, 0])
    with pytest.raises(ValueError, match="at least one cloud"):
        m.forward_packed(x, [])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.forward_packed(x, [4, 6])

