"""tests/cloud_model.py — the longdouble reference of the resident data set kernel tests — held to what the reference
project's fixtures already pin: Building3DReconstructionDataset on the fixture clouds (tests/test_dataset.py compares it
with the reference's own items) and wf3d.targets.train_targets.  CPU only; nothing here runs a kernel."""
import os
import types

import numpy as np
import pytest

import helpers as H
import cloud_cases as K
import cloud_model as M

ROOT = os.path.join(H.GOLDEN, "building3d")
TOL = 1e-6                                               # tests/test_dataset.py: device batches against host batches


def _dataset(augment, use_color=True, use_intensity=True):
    from datasets import Building3DReconstructionDataset
    cfg = types.SimpleNamespace(root_dir=ROOT, num_points=0, use_color=use_color, use_intensity=use_intensity, normalize=True,
                                augment=augment)
    return Building3DReconstructionDataset(cfg, split_set="train")


@pytest.mark.parametrize("augment", [False, True])
@pytest.mark.parametrize("C", [8, 7, 3])
def test_model_reproduces_the_host_data_set_on_the_fixture_clouds(C, augment):
    from datasets.building3d import load_wireframe
    ds = _dataset(augment, use_color=C > 3, use_intensity=C > 7)
    assert len(ds) == 2
    raws = [np.loadtxt(f, dtype=np.float64)[:, :C] for f in ds.pc_files]
    raw, first = K.packed(raws)
    norm, cen, md = M.normalize_model(raw, first, C, *K.COLOR_RANGE[C], 1)
    wfs = [load_wireframe(f) for f in ds.wireframe_files]
    wfs = [((v.astype(M.LD) - cen[i]) / md[i], e) for i, (v, e) in enumerate(wfs)]
    wfv, wfe, vfirst, efirst = K.resident_wireframes([(v.astype(np.float64), e) for v, e in wfs])
    idxs = [1, 0, 1]
    np.random.seed(17)
    items = [ds[i] for i in idxs]
    np.random.seed(17)
    draws = [ds._draw_augmentation() if augment else (1.0, 1.0, 0.0) for _ in idxs]
    aug = np.array([(fx, fy, np.cos(t), np.sin(t)) for fx, fy, t in draws]).reshape(len(idxs), 4)
    out_first = np.concatenate([[0], np.cumsum([raws[i].shape[0] for i in idxs])])
    capacity = int(out_first[-1]) + 3
    points, counts = M.gather_model(norm.astype(np.float64), first, idxs, None, aug, out_first, capacity)
    assert counts.tolist() == [raws[i].shape[0] for i in idxs] and not points[out_first[-1]:].any()
    choice = [np.arange(0, raws[i].shape[0], 7)[:150] for i in idxs]
    sampled = M.gather_model(norm.astype(np.float64), first, idxs, np.stack(choice), aug)
    V = 16
    tg = M.targets_model(wfv, wfe, vfirst, efirst, idxs, aug, V)
    for b, (i, it) in enumerate(zip(idxs, items)):
        pc = it["point_clouds"]
        assert pc.dtype == np.float32 and pc.shape == (raws[i].shape[0], C)
        err = float(np.abs(points[out_first[b]:out_first[b + 1]].astype(np.float64) - pc).max())
        assert err < TOL, (b, err)
        assert float(np.abs(sampled[b].astype(np.float64) - pc[choice[b]]).max()) < TOL
        assert np.allclose(np.asarray(cen[i], dtype=np.float64), it["centroid"], rtol=0, atol=TOL)
        assert abs(float(md[i]) - float(it["max_distance"])) < TOL
        c = it["wf_vertices"].shape[0]
        assert tg["vertex_counts"][b] == c and float(np.abs(tg["vertices"][b, :c] - it["wf_vertices"]).max()) < TOL
        assert not tg["vertices"][b, c:].any()


def _host_targets(wfs, cloud, aug, V):
    """train_targets of the samples' wireframes with the flips applied on the host in float64 (exact)"""
    from wf3d.targets import train_targets
    vs, es = [], []
    for b, cl in enumerate(cloud):
        v = wfs[cl][0].copy()
        v[:, 0] *= aug[b, 0]
        v[:, 1] *= aug[b, 1]
        vs.append(v)
        es.append(wfs[cl][1])
    return train_targets(vs, es, V, full_width=True)


@pytest.mark.parametrize("kind", ["identity", "flips"])
@pytest.mark.parametrize("V", [1, 2, 3, 16, 17, 300])
def test_targets_model_is_train_targets(V, kind):
    wfs, names = K.wireframes()
    wfv, wfe, vfirst, efirst = K.resident_wireframes(wfs)
    cloud = [i for i, (v, _) in enumerate(wfs) if v.shape[0] <= V]
    cloud = cloud + cloud[::-1][:2]                                   # a repeated wireframe
    aug = K.augmentation(kind, len(cloud))
    got = M.targets_model(wfv, wfe, vfirst, efirst, cloud, aug, V)
    want = _host_targets(wfs, cloud, aug, V)
    for k, w in want.items():
        w = w.numpy()
        assert got[k].dtype == w.dtype and got[k].shape == w.shape, k
        assert np.array_equal(got[k].view(np.int32 if w.dtype == np.float32 else w.dtype),
                              w.view(np.int32 if w.dtype == np.float32 else w.dtype)), k
    if V >= 16:                                                       # the edge lists do what their names say
        b = cloud.index(names["c16_all"])
        assert got["edge_labels"][b, :120].all() and not got["edge_labels"][b, 120:].any()
        b = cloud.index(names["c16_mixed"])
        assert 0 < got["edge_labels"][b].sum() < 120


def test_targets_model_clamps_and_zeroes_as_the_header_says():
    wfs, names = K.wireframes()
    wfv, wfe, vfirst, efirst = K.resident_wireframes(wfs)
    cloud = [names["c17"], -1, len(wfs), names["c3_all_reversed"]]
    got = M.targets_model(wfv, wfe, vfirst, efirst, cloud, K.augmentation("identity", 4), 16)
    assert got["vertex_counts"].tolist() == [17, 0, 0, 3]
    assert got["vertex_existence"].sum(axis=1).tolist() == [16, 0, 0, 3]
    v17, e17 = wfs[names["c17"]]
    assert np.array_equal(got["vertices"][0], v17[:16].astype(np.float32))
    lab = np.zeros(120, np.float32)
    for a, d in e17.tolist():
        if 0 <= min(a, d) < max(a, d) < 16:
            lab[M.pair_index(min(a, d), max(a, d), 16)] = 1.0
    assert np.array_equal(got["edge_labels"][0], lab) and 10 < lab.sum() < len(e17)      # some edges reach vertex 16: dropped
    assert not got["vertices"][1:3].any() and not got["edge_labels"][1:3].any()
    assert got["edge_labels"][3, :3].all() and not got["edge_labels"][3, 3:].any()


def test_gather_model_zeroes_what_lies_outside():
    rng = np.random.RandomState(1)
    norm = rng.uniform(-1, 1, (10, 3))
    first = [0, 4, 4, 10]
    aug = K.augmentation("identity", 3)
    got = M.gather_model(norm, first, [2, 1, 3], [[0, 5, 6, -1], [0, 0, 0, 0], [0, 1, 2, 3]], aug)
    assert np.array_equal(got[0, :2], norm[[4, 9]].astype(np.float32)) and not got[0, 2:].any() and not got[1:].any()
    pts, counts = M.gather_model(norm, first, [0, 1, 2], None, aug, [2, 6, 6, 9], 12)
    assert counts.tolist() == [4, 0, 6]
    assert not pts[:2].any() and np.array_equal(pts[2:6], norm[0:4].astype(np.float32))
    assert np.array_equal(pts[6:9], norm[4:7].astype(np.float32)) and not pts[9:].any()
    # a span longer than its cloud: zeros behind the cloud's rows
    pts, _ = M.gather_model(norm, first, [0, 2], None, K.augmentation("identity", 2), [0, 6, 12], 12)
    assert np.array_equal(pts[:4], norm[:4].astype(np.float32)) and not pts[4:6].any() and np.array_equal(pts[6:], norm[4:].astype(np.float32))
