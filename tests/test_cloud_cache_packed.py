"""The host plan of a packed batch from resident clouds (datasets.building3d.packed_plan: what DeviceCloudCache.stage and
packed_batch do before any launch) on the fixture clouds of tests/golden/building3d, without a GPU: output-row offsets,
the refusals (nothing drawn before them), index handling, and np.random left as the host data set with num_points = 0
leaves it."""
import os
import types

import numpy as np
import pytest

import helpers as H

ROOT = os.path.join(H.GOLDEN, "building3d")
POINTS = {"100": 1276, "10040": 1504}
VERTICES = {"100": 8, "10040": 4}


def _ds0(augment):
    from datasets import Building3DReconstructionDataset
    cfg = types.SimpleNamespace(root_dir=ROOT, num_points=0, use_color=True, use_intensity=True, normalize=True, augment=augment)
    return Building3DReconstructionDataset(cfg, split_set="train")


def _sizes(ds):
    from datasets.building3d import load_wireframe
    names = [os.path.splitext(os.path.basename(f))[0] for f in ds.pc_files]
    n = [ds[i]["point_clouds"].shape[0] for i in range(len(ds))]
    nv = [load_wireframe(f)[0].shape[0] for f in ds.wireframe_files]
    assert [POINTS[k] for k in names] == n and [VERTICES[k] for k in names] == nv
    return names, n, nv


@pytest.mark.parametrize("indices", [[0, 1], [1, 1, 0], [0, 1, 1, 0, 1]], ids=str)
def test_offsets(indices):
    from datasets.building3d import packed_plan
    _, n, nv = _sizes(_ds0(False))
    idx, out_first, aug = packed_plan(n, nv, indices)
    assert idx == indices and out_first.dtype == np.int32 and aug.dtype == np.float64
    assert out_first.tolist() == [0] + np.cumsum([n[i] for i in indices]).tolist()
    assert np.array_equal(aug, np.tile([1.0, 1.0, 1.0, 0.0], (len(indices), 1)))
    # the tightest capacity and max_vertices pass
    packed_plan(n, nv, indices, capacity=int(out_first[-1]), max_vertices=8)


def test_refusals_come_before_any_draw():
    from datasets.building3d import packed_plan
    ds = _ds0(True)
    names, n, nv = _sizes(ds)
    np.random.seed(3)
    state = np.random.get_state()[1].copy()
    with pytest.raises(ValueError, match="hold 2780 points, above the capacity of 2560 rows"):
        packed_plan(n, nv, [0, 1], ds._draw_augmentation, capacity=2560, max_vertices=8)
    with pytest.raises(ValueError, match="a wireframe has 8 vertices, more than max_vertices = 4"):
        packed_plan(n, nv, [names.index("100")], ds._draw_augmentation, capacity=2560, max_vertices=4)
    packed_plan(n, nv, [names.index("10040")], None, capacity=2560, max_vertices=4)
    with pytest.raises(ValueError, match="empty batch"):
        packed_plan(n, nv, [], ds._draw_augmentation)
    assert np.array_equal(np.random.get_state()[1], state)


def test_indices():
    from datasets.building3d import packed_plan
    _, n, nv = _sizes(_ds0(False))
    assert packed_plan(n, nv, [-1, -2, np.int64(0)])[0] == [1, 0, 0]
    assert packed_plan(n, nv, [-1, -2])[1].tolist() == [0, n[1], n[1] + n[0]]
    for bad in ([2], [0, -3], [0, 10 ** 12]):
        with pytest.raises(IndexError, match="index out of range for 2 clouds"):
            packed_plan(n, nv, bad)
    with pytest.raises(TypeError):
        packed_plan(n, nv, [0.5])


@pytest.mark.parametrize("augment", [False, True])
@pytest.mark.parametrize("seed,indices", [(5, [0, 1]), (6, [1, 1, 0])], ids=str)
def test_random_state_follows_the_host_data_set(augment, seed, indices):
    """and, when augmenting, the drawn parameters are those the host items were built with"""
    from datasets.building3d import packed_plan
    ds = _ds0(augment)
    _, n, nv = _sizes(ds)
    np.random.seed(seed)
    items = [ds[i] for i in indices]
    want_next = np.random.random()
    np.random.seed(seed)
    _, out_first, aug = packed_plan(n, nv, indices, ds._draw_augmentation if augment else None)
    assert np.random.random() == want_next
    assert out_first.tolist() == [0] + np.cumsum([it["point_clouds"].shape[0] for it in items]).tolist()
    np.random.seed(seed)
    for a in aug:
        fx, fy, angle = ds._draw_augmentation() if augment else (1.0, 1.0, 0.0)
        assert a.tolist() == [fx, fy, np.cos(angle), np.sin(angle)]
    assert np.allclose(aug[:, 2] ** 2 + aug[:, 3] ** 2, 1.0, rtol=0, atol=1e-15)
