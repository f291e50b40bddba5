"""Packed batches in the capacity form, the parts that need no GPU: the host table of ops.PackedLayout(counts, capacity=)
(include/wf3d.h, "PACKED batches, capacity form"), its sizing against wf3d_packed_layout_dims, pack_into, and the C ABI."""
import ctypes
import os

import numpy as np
import pytest
import torch

import helpers as H

ODD = [255, 256, 257, 1, 513]                       # sum 1282
CASES = [(ODD, 1536), (ODD, 2048), ([256, 512, 768], 1536), ([1], 256), ([300], 512), ([512], 512),
         ([14039, 1276, 64], 3 * 14080), ([4096] * 32, 131072)]


@pytest.mark.parametrize("counts,capacity", CASES)
def test_capacity_table_invariants(counts, capacity):
    from wf3d.ops import PackedLayout, capacity_dims, chunk_rows_of
    lay = PackedLayout(counts, capacity=capacity)
    B, M = len(counts), sum(counts)
    cr, ncap = capacity_dims(B, capacity)
    assert cr == chunk_rows_of(capacity) == max(256, -(-(-(-capacity // 256)) // 64) * 64)
    assert ncap == -(-capacity // cr) + B + 1
    assert (lay.M, lay.M_pad, lay.M_abi, lay.capacity, lay.chunk_rows) == (M, capacity, capacity, capacity, cr)
    assert lay.offsets.tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist()
    ck = lay.chunks
    assert ck.shape == (ncap, 4) and lay.nchunk == lay.nchunk_bwd == ncap          # the table length is nchunk_cap
    # the chunks tile 0 .. capacity exactly once, in row order, none longer than chunk_rows
    live = ck[ck[:, 3] > ck[:, 2]]
    assert live[0, 2] == 0 and live[-1, 3] == capacity
    assert np.array_equal(live[1:, 2], live[:-1, 3])
    assert np.all(ck[:, 3] - ck[:, 2] <= cr) and np.all(ck[:, 3] >= ck[:, 2])
    # cloud chunks: consecutive, in row order, inside their cloud, located by chunk_offsets
    co = lay.chunk_offsets
    assert co[0] == 0 and len(co) == B + 1
    for b in range(B):
        mine = ck[co[b]:co[b + 1]]
        assert len(mine) == -(-counts[b] // cr)
        assert np.all(mine[:, 0] == b) and np.all(mine[:, 1] == lay.offsets[b])
        assert mine[0, 2] == lay.offsets[b] and mine[-1, 3] == lay.offsets[b + 1]
    # then the pad rows in pieces, then dead entries (capacity, capacity)
    rest = ck[co[B]:]
    assert np.all(rest[:, 0] == -1) and np.all(rest[:, 1] == 0)
    npad = -(-(capacity - M) // cr)
    assert np.all(rest[:npad, 3] > rest[:npad, 2]) and (npad == 0 or (rest[0, 2] == M and rest[npad - 1, 3] == capacity))
    assert np.all(rest[npad:, 2:] == capacity)
    if M == capacity:
        assert npad == 0 and len(rest) >= 1                                         # a full batch: dead entries only
    rm = lay.row_map()
    assert rm.shape == (capacity,) and np.all(rm[M:] == -1) and np.all(rm[:M] >= 0)


def test_capacity_does_not_change_the_plain_layout():
    from wf3d.ops import PackedLayout
    a = PackedLayout(ODD)
    assert a.capacity is None and a.M_abi == a.M == 1282 and a.M_pad == 1536 and a.status is None
    assert a.nchunk_bwd == a.nchunk + 1 and a.chunks[-1].tolist() == [-1, 0, 1282, 1536]
    # at chunk_rows 256 the clouds' chunks of the capacity table are the plain layout's
    b = PackedLayout(ODD, capacity=2048)
    assert np.array_equal(b.chunks[:a.nchunk], a.chunks[:a.nchunk]) and np.array_equal(a.chunk_offsets, b.chunk_offsets)


def test_capacity_errors():
    from wf3d.ops import PackedLayout
    with pytest.raises(ValueError, match="above the capacity"):
        PackedLayout(ODD, capacity=1280)
    for bad in (1000, 255, 0, -256, 256.0):
        with pytest.raises(ValueError, match="multiple of 256|must be an int"):
            PackedLayout([5, 7], capacity=bad)
    with pytest.raises(ValueError, match="at least one point"):
        PackedLayout([5, 0], capacity=256)


def test_cache_key_includes_capacity(monkeypatch):
    from wf3d.ops import PackedLayout
    monkeypatch.setattr(PackedLayout, "to", lambda self, device: self)
    monkeypatch.setattr(PackedLayout, "use", lambda self: self)
    monkeypatch.setattr(PackedLayout, "_cache", {})
    d = torch.device("cuda:0")
    a, b, c = PackedLayout.get([5, 7], d), PackedLayout.get([5, 7], d, 256), PackedLayout.get([5, 7], d, 512)
    assert a.capacity is None and b.capacity == 256 and c.capacity == 512
    assert PackedLayout.get([5, 7], d, 256) is b and PackedLayout.get([5, 7], d) is a and len(PackedLayout._cache) == 3


def test_pack_into():
    from wf3d.packed import pack_into
    g = torch.Generator().manual_seed(0)
    clouds = [torch.randn(n, 8, generator=g) for n in (5, 1, 7)]
    pts, cnt = torch.full((256, 8), 9.0), torch.zeros(3, dtype=torch.int64)
    assert pack_into(pts, cnt, clouds) == [5, 1, 7]
    assert cnt.tolist() == [5, 1, 7] and torch.equal(pts[:13], torch.cat(clouds)) and float(pts[13:].abs().max()) == 0.0
    c32 = torch.zeros(3, dtype=torch.int32)
    pack_into(pts, c32, [c.numpy() for c in clouds[::-1]])
    assert c32.tolist() == [7, 1, 5] and c32.dtype == torch.int32
    with pytest.raises(ValueError, match="above the capacity"):
        pack_into(pts, cnt, [torch.randn(200, 8), torch.randn(50, 8), torch.randn(7, 8)])
    with pytest.raises(ValueError, match="3 clouds|2 clouds"):
        pack_into(pts, cnt, clouds[:2])
    with pytest.raises(ValueError, match="columns"):
        pack_into(pts, cnt, [torch.randn(3, 4)] * 3)
    with pytest.raises(ValueError):
        pack_into(pts, torch.zeros(3), clouds)
    assert cnt.tolist() == [5, 1, 7]                                                # a refused call wrote nothing


def test_symbols_in_header_and_loader_and_dims_agree_with_python():
    from wf3d import _lib
    from wf3d.ops import capacity_dims
    hdr = open(os.path.join(H.ROOT, "include", "wf3d.h")).read()
    lib = _lib.load()
    for n in ("wf3d_packed_layout_dims", "wf3d_packed_layout_build", "wf3d_packed_layout_build_i32"):
        assert n + "(" in hdr and n in _lib.SIGNATURES and hasattr(lib, n)
    cr, nc = ctypes.c_int(), ctypes.c_int()
    for B, cap in [(1, 256), (3, 1536), (5, 2048), (3, 3 * 14080), (32, 131072), (65535, 256), (7, 0x7FFFFF00)]:
        assert lib.wf3d_packed_layout_dims(B, cap, ctypes.byref(cr), ctypes.byref(nc)) == 0
        assert (cr.value, nc.value) == capacity_dims(B, cap), (B, cap)
    for B, cap in [(0, 256), (65536, 256), (3, 0), (3, 1000), (3, -256)]:
        assert lib.wf3d_packed_layout_dims(B, cap, ctypes.byref(cr), ctypes.byref(nc)) != 0
    # the builder's argument checks are reachable without a GPU (no kernel is launched)
    assert lib.wf3d_packed_layout_build(None, 3, 1536, None, None, None, None, None) != 0
    assert b"null pointer" in lib.wf3d_last_error()
    assert lib.wf3d_packed_layout_build_i32(None, 3, 1000, None, None, None, None, None) != 0
    assert b"multiple of 256" in lib.wf3d_last_error()


def test_surface_takes_capacity():
    import inspect
    from models.PointCloudToWireframe import PointCloudToWireframe
    from models.PointNetEncoder import PointNetEncoder
    assert list(inspect.signature(PointNetEncoder.encode_packed).parameters)[1:] == ["points", "point_counts", "capacity"]
    assert list(inspect.signature(PointCloudToWireframe.forward_packed).parameters)[1:] == [
        "points", "point_counts", "target_vertex_counts", "capacity"]
    enc = PointNetEncoder(8, [32, 64], 16)
    with pytest.raises(ValueError, match="multiple of 256"):
        enc.encode_packed(torch.zeros(1000, 8), [5, 7], capacity=1000)
    with pytest.raises(ValueError, match="must have 512 rows"):
        enc.encode_packed(torch.zeros(256, 8), [5, 7], capacity=512)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        enc.encode_packed(torch.zeros(256, 8), [5, 7], capacity=256)
