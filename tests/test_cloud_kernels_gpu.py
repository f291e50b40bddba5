"""The resident data set kernels of csrc/cloud.hip — wf3d_cloud_normalize, wf3d_cloud_sample, wf3d_cloud_pack,
wf3d_wireframe_targets — called through their C entry points on synthetic, seeded, building-like clouds (UTM offsets,
4 decimals) and wireframes, against the longdouble model of tests/cloud_model.py, which tests/test_cloud_model.py holds to
the host data set.  Parameter blocks are built by hand in include/wf3d.h's layout; every output buffer is poisoned and
sits between guard elements that must stay untouched.

Normalise tolerance, derived (u = 2^-53, k = ceil(n / 256) + 8 the longest chain of additions a term passes through in
the kernel — n / 256 strided partial sums per lane, a tree of 8 —, M = max |raw xyz| of the cloud, md its max-norm):
    centroid      (k + 1) u M
    max_distance  sqrt(3) (k + 1) u M + 4 u md
    xyz rows      3 (k + 1) u M / md + 8 u
1e-9 .. 3e-9 in normalised units for these clouds; a float32 slip anywhere is >= 1e-2.  Colour and further columns: exact.
The gathers (sample, pack, targets) are compared with the model applied to the table the device normalised, read back:
identity and flips bit for bit in every column, a rotation within one float32 spacing in x and y (the fp64 expression
may be contracted to an fma and is rounded twice, to fp64 and to fp32) and bit for bit elsewhere.  NaN (the xyz of the
one-row cloud, 0 / 0) matches NaN."""
import functools
import glob
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import helpers as H  # noqa: E402
import cloud_cases as K  # noqa: E402
import cloud_model as M  # noqa: E402

GUARD = 64                     # elements in front of and behind every output (a multiple of 16 bytes for every type)
U = 2.0 ** -53
AUG_KINDS = ("identity", "flips", "rotation")


def dev():
    return torch.device("cuda:0")


def _lib():
    from wf3d import _lib
    return _lib.load()


def _check(code, what):
    from wf3d import _lib
    _lib.check(code, what)


def _stream():
    from wf3d.ops import _stream
    return _stream()


class Guarded:
    """a poisoned output `t` of `shape` inside one allocation with GUARD poisoned elements on either side"""

    def __init__(self, shape, dtype):
        self.n = int(np.prod(shape, dtype=np.int64))
        self.poison = 7.0 if dtype.is_floating_point else -7
        self.buf = torch.full((self.n + 2 * GUARD,), self.poison, dtype=dtype, device=dev())
        self.t = self.buf[GUARD:GUARD + self.n].view(*shape)

    def ptr(self):
        return self.t.data_ptr()

    def read(self):
        """the output on the host; asserts the guards untouched"""
        whole = self.buf.cpu()
        assert bool((whole[:GUARD] == self.poison).all()) and bool((whole[GUARD + self.n:] == self.poison).all()), "guard elements written"
        return whole[GUARD:GUARD + self.n].view(*self.t.shape).numpy()


def _to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _block(aug, cloud, out_first):
    """the parameter block of include/wf3d.h on the device: aug [B, 4] doubles, cloud [B] ints at byte 32 B, out_first
    [B + 1] ints at byte 36 B"""
    B = len(cloud)
    raw = np.zeros(40 * B + 4, dtype=np.uint8)
    raw[:32 * B].view(np.float64)[:] = np.asarray(aug, dtype=np.float64).reshape(-1)
    raw[32 * B:36 * B].view(np.int32)[:] = cloud
    raw[36 * B:].view(np.int32)[:] = out_first
    return _to_dev(raw)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


def _check_rows(got, want, rotated, what):
    """float32 rows [..., C]: NaN where the model has NaN; elsewhere bit for bit, except x and y under a rotation, which
    stay within one float32 spacing.  Returns the largest |x, y difference| in spacings."""
    assert got.dtype == np.float32 and got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    g, w = np.where(nan, np.float32(0), got), np.where(nan, np.float32(0), want)
    lo = 2 if rotated else 0
    assert np.array_equal(_bits(g[..., lo:]), _bits(w[..., lo:])), what
    if not rotated:
        return 0.0
    gx, wx = g[..., :2].astype(np.float64), w[..., :2].astype(np.float64)
    spacing = np.maximum(np.spacing(np.abs(w[..., :2])), np.spacing(np.abs(g[..., :2]))).astype(np.float64)
    worst = float((np.abs(gx - wx) / spacing).max()) if gx.size else 0.0
    assert worst <= 1.0, (what, worst)
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# 1. normalise
# ---------------------------------------------------------------------------------------------------------------------
def _normalize(raw, first, C, lo, hi, normalize):
    """one launch into poisoned, guarded outputs -> (out [rows, C], centroid [ncl, 3], max_distance [ncl]) float64"""
    ncl = len(first) - 1
    out, cen, md = Guarded((raw.shape[0], C), torch.float64), Guarded((ncl, 3), torch.float64), Guarded((ncl,), torch.float64)
    d_raw, d_first = _to_dev(raw), _to_dev(first)
    _check(_lib().wf3d_cloud_normalize(d_raw.data_ptr(), d_first.data_ptr(), ncl, C, lo, hi, normalize, out.ptr(), cen.ptr(), md.ptr(),
                                       _stream()), "cloud_normalize")
    return out.read(), cen.read(), md.read(), out


def _bounds(raw_xyz, n, md):
    k = math.ceil(n / 256) + 8
    big = float(np.abs(raw_xyz).max())
    return (k + 1) * U * big, math.sqrt(3) * (k + 1) * U * big + 4 * U * md, 3 * (k + 1) * U * big / md + 8 * U


def _check_normalized(raw, first, C, got, want):
    """every cloud against the longdouble model within the derived bounds; prints and returns the observed maxima"""
    (g_out, g_cen, g_md), (w_out, w_cen, w_md) = got, want
    assert np.array_equal(_bits(g_out[:, 3:]), _bits(w_out[:, 3:].astype(np.float64)))          # colour / 256 is exact
    worst = {"centroid": (0.0, 1.0), "max_distance": (0.0, 1.0), "rows": (0.0, 1.0)}
    for i in range(len(first) - 1):
        lo, hi = int(first[i]), int(first[i + 1])
        n = hi - lo
        if n == 0:
            continue
        if n == 1:                                       # pinned: the centroid is the row, max-norm 0, xyz 0 / 0
            assert np.array_equal(g_cen[i], raw[lo, :3]) and g_md[i] == 0.0 and np.isnan(g_out[lo, :3]).all()
            assert np.isnan(w_out[lo, :3]).all() and w_md[i] == 0
            continue
        b_cen, b_md, b_rows = _bounds(raw[lo:hi, :3], n, float(w_md[i]))
        errs = {"centroid": (float(np.abs(g_cen[i].astype(M.LD) - w_cen[i]).max()), b_cen),
                "max_distance": (float(abs(M.LD(g_md[i]) - w_md[i])), b_md),
                "rows": (float(np.abs(g_out[lo:hi, :3].astype(M.LD) - w_out[lo:hi, :3]).max()), b_rows)}
        for k, (e, b) in errs.items():
            assert e <= b, (i, n, k, e, b)
            if e / b >= worst[k][0] / worst[k][1]:
                worst[k] = (e, b)
    print("normalise C=%d: " % C + ", ".join("%s %.2e (bound %.2e)" % (k, e, b) for k, (e, b) in worst.items()))
    return worst


@functools.lru_cache(maxsize=None)
def _resident(C):
    """the synthetic clouds of cloud_cases.normalize_clouds(C), normalised by ONE launch: the inputs, the device table
    (kept on the device for the gathers), its read-back and the model"""
    clouds, names = K.normalize_clouds(C)
    raw, first = K.packed(clouds)
    lo, hi = K.COLOR_RANGE[C]
    g_out, g_cen, g_md, keep = _normalize(raw, first, C, lo, hi, 1)
    want = M.normalize_model(raw, first, C, lo, hi, 1)
    return dict(raw=raw, first=first, names=names, got=(g_out, g_cen, g_md), want=want, table=keep.t, d_first=_to_dev(first),
                ncl=len(clouds))


@pytest.mark.parametrize("C", [3, 7, 8, 4, 16])
def test_normalize_every_row_count_against_the_longdouble_model(C):
    r = _resident(C)
    first, names = r["first"], r["names"]
    e = names["empty"]
    assert first[e] == first[e + 1] and 0 < e < r["ncl"] - 1           # a cloud of no rows between two others
    assert [int(first[names[n] + 1] - first[names[n]]) for n in K.ROWS] == list(K.ROWS)
    _check_normalized(r["raw"], first, C, r["got"], r["want"])
    g_out = r["got"][0]
    for row in (0, 512, 255, 256):                                      # the planted point is the farthest: its norm is 1
        i = names[f"far{row}"]
        lo = int(first[i])
        norms = np.sqrt((r["want"][0][lo:lo + 513, :3] ** 2).sum(axis=1))
        assert int(np.argmax(norms)) == row and float(norms[row]) == pytest.approx(1.0, abs=1e-15)
        got_norms = np.sqrt((g_out[lo:lo + 513, :3] ** 2).sum(axis=1))
        assert int(np.argmax(got_norms)) == row and abs(float(got_norms[row]) - 1.0) < 1e-8 and float(np.delete(got_norms, row).max()) < 0.5


def test_normalize_off_passes_rows_through():
    clouds, names = K.normalize_clouds(8)
    raw, first = K.packed(clouds)
    g_out, g_cen, g_md, _ = _normalize(raw, first, 8, 3, 7, 0)
    want = raw.copy()
    want[:, 3:7] /= 256.0
    assert np.array_equal(_bits(g_out), _bits(want))
    assert (g_cen == 7.0).all() and (g_md == 7.0).all()                 # not written
    # without a colour range nothing is scaled; centroid / max_distance may be NULL
    out = Guarded(raw.shape, torch.float64)
    d_raw, d_first = _to_dev(raw), _to_dev(first)
    _check(_lib().wf3d_cloud_normalize(d_raw.data_ptr(), d_first.data_ptr(), len(clouds), 8, 0, 0, 0, out.ptr(), None, None, _stream()),
           "cloud_normalize")
    assert np.array_equal(_bits(out.read()), _bits(raw))


def test_normalize_fixture_clouds_within_the_derived_bound():
    """real UTM data: the three fixture clouds, same bound"""
    files = sorted(glob.glob(os.path.join(H.GOLDEN, "building3d", "*", "xyz", "*.xyz")))
    assert len(files) == 3
    raw, first = K.packed([np.loadtxt(f, dtype=np.float64) for f in files])
    assert raw.shape[1] == 8 and float(np.abs(raw[:, :3]).max()) > 6e6
    g_out, g_cen, g_md, _ = _normalize(raw, first, 8, 3, 7, 1)
    _check_normalized(raw, first, 8, (g_out, g_cen, g_md), M.normalize_model(raw, first, 8, 3, 7, 1))


# ---------------------------------------------------------------------------------------------------------------------
# 2. the host-choice sampler
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", AUG_KINDS)
@pytest.mark.parametrize("C", [8, 3])
@pytest.mark.parametrize("P", [1, 255, 256, 257])
def test_sample_gathers_and_rounds_once(P, C, kind):
    r = _resident(C)
    first, names = r["first"], r["names"]
    cloud = [names[257], names[2], names[1300]]
    B = len(cloud)
    rng = np.random.RandomState(P)
    choice = np.empty((B, P), dtype=np.int32)
    for b, cl in enumerate(cloud):
        n = int(first[cl + 1] - first[cl])
        choice[b] = rng.randint(0, n, P)
        if P == 1:
            choice[b, 0] = (0, n - 1, n // 2)[b]
        else:
            choice[b, [0, 1, 2, 3, P - 1]] = [0, n - 1, n // 2, n // 2, n - 1]      # the first row, the last, repeats
    aug = K.augmentation(kind, B, seed=P)
    out = Guarded((B, P, C), torch.float32)
    d_cloud, d_choice, d_aug = _to_dev(np.asarray(cloud, dtype=np.int32)), _to_dev(choice), _to_dev(aug)
    _check(_lib().wf3d_cloud_sample(r["table"].data_ptr(), r["d_first"].data_ptr(), d_cloud.data_ptr(), d_choice.data_ptr(),
                                    d_aug.data_ptr(), B, P, C, out.ptr(), _stream()), "cloud_sample")
    want = M.gather_model(r["got"][0], first, cloud, choice, aug)
    assert not np.isnan(want).any() and np.abs(want[..., :3]).max() <= 1.001
    worst = _check_rows(out.read(), want, kind == "rotation", (P, C, kind))
    print(f"sample P={P} C={C} {kind}: x, y within {worst:.2f} float32 spacings of the model")


# ---------------------------------------------------------------------------------------------------------------------
# 3. pack
# ---------------------------------------------------------------------------------------------------------------------
def _pack(r, C, cloud, out_first, capacity, aug):
    """one wf3d_cloud_pack launch on the resident table into guarded outputs -> (points, point_counts)"""
    B = len(cloud)
    block = _block(aug, cloud, out_first)
    points, counts = Guarded((capacity, C), torch.float32), Guarded((B,), torch.int64)
    _check(_lib().wf3d_cloud_pack(r["table"].data_ptr(), r["d_first"].data_ptr(), r["ncl"], block.data_ptr(), B, capacity, C,
                                  points.ptr(), counts.ptr(), _stream()), "cloud_pack")
    return points.read(), counts.read()


def _spans(r, cloud):
    first = r["first"]
    return np.concatenate([[0], np.cumsum([int(first[c + 1] - first[c]) for c in cloud])]).astype(np.int64)


def _pack_and_compare(r, C, cloud, out_first, capacity, kind, what):
    aug = K.augmentation(kind, len(cloud), seed=len(cloud))
    points, counts = _pack(r, C, cloud, out_first, capacity, aug)
    want, want_counts = M.gather_model(r["got"][0], r["first"], cloud, None, aug, out_first, capacity)
    assert counts.dtype == np.int64 and np.array_equal(counts, want_counts), what
    _check_rows(points, want, kind == "rotation", what)
    return points, counts


@pytest.mark.parametrize("kind", AUG_KINDS)
@pytest.mark.parametrize("C", [8, 7, 3])
def test_pack_boundaries_at_odd_and_even_rows(C, kind):
    r = _resident(C)
    cloud = [r["names"][n] for n in (257, 1, 255, 256, 2)]
    out_first = _spans(r, cloud)
    assert out_first.tolist() == [0, 257, 258, 513, 769, 771]
    points, counts = _pack_and_compare(r, C, cloud, out_first, 1024, kind, "capacity 1024")
    assert counts.tolist() == [257, 1, 255, 256, 2] and not points[771:].any() and np.isnan(points[257, :3]).all()
    assert bool((points[:257] != 0).any(axis=1).all())
    _pack_and_compare(r, C, cloud, out_first, 771, kind, "capacity 771: no tail, no multiple of 256")


@pytest.mark.parametrize("C", [8, 7, 3])
def test_pack_grid_sized_by_the_batch(C):
    """B = 700 samples of the one-row cloud into 256 rows: rows 0 .. 255 written and nothing behind them, 700 counts"""
    r = _resident(C)
    one = r["names"][1]
    points, counts = _pack_and_compare(r, C, [one] * 700, np.arange(701), 256, "flips", "B = 700")
    assert (counts == 1).all() and np.isnan(points[:, :3]).all()
    if C > 3:
        src = r["got"][0][int(r["first"][one]), 3:].astype(np.float32)
        assert np.array_equal(points[:, 3:], np.tile(src, (256, 1)))


@pytest.mark.parametrize("C", [8, 7, 3])
def test_pack_largest_batch_repeats_and_one_sample(C):
    r = _resident(C)
    names = r["names"]
    rng = np.random.RandomState(4096)
    cloud = [names[int(n)] for n in rng.randint(1, 4, 4096)]            # 4096 samples of the 1-, 2- and 3-row clouds
    out_first = _spans(r, cloud)
    for kind in ("flips", "rotation"):
        _pack_and_compare(r, C, cloud, out_first, int(out_first[-1]) + 3, kind, "B = 4096")
        cloud2 = [names[257], names[3], names[257], names[257]]         # a repeated cloud
        _pack_and_compare(r, C, cloud2, _spans(r, cloud2), 800, kind, "repeats")
        _pack_and_compare(r, C, [names[513]], [0, 513], 513, kind, "B = 1")
        _pack_and_compare(r, C, [names[2]], [0, 2], 1, kind, "B = 1, capacity 1")


@pytest.mark.parametrize("C", [8, 7, 3])
def test_pack_empty_clouds(C):
    """a cloud of no rows (first[i] == first[i+1], which no file gives) owns no output row; its count is 0"""
    r = _resident(C)
    n = r["names"]
    a, b, e = n[257], n[2], n["empty"]
    for kind in ("flips", "rotation"):
        for cloud in ([a, e, b], [e, a], [a, e], [e, e, b, e]):
            out_first = _spans(r, cloud)
            points, counts = _pack_and_compare(r, C, cloud, out_first, int(out_first[-1]) + 5, kind, cloud)
            assert [int(c) for c in counts] == [0 if c == e else int(r["first"][c + 1] - r["first"][c]) for c in cloud]
            assert bool((points[:int(out_first[-1])] != 0).any(axis=1).all()) and not points[int(out_first[-1]):].any()


@pytest.mark.parametrize("C", [8, 7, 3])
def test_pack_blocks_that_break_the_rules_give_zero_rows(C):
    r = _resident(C)
    n, ncl = r["names"], r["ncl"]
    for kind in ("flips", "rotation"):
        # cloud indices outside the resident clouds: their rows are zeros, their counts 0
        cloud, out_first = [n[257], -1, n[2], ncl, n[3]], [0, 257, 261, 263, 267, 270]
        points, counts = _pack_and_compare(r, C, cloud, out_first, 300, kind, "unknown clouds")
        assert counts.tolist() == [257, 0, 2, 0, 3] and not points[257:261].any() and not points[263:267].any()
        assert bool((points[261:263] != 0).any()) and bool((points[267:270] != 0).any())
        # a span longer than its cloud: zeros behind the cloud's rows
        points, counts = _pack_and_compare(r, C, [n[3], n[257]], [0, 10, 267], 267, kind, "long span")
        assert counts.tolist() == [3, 257] and not points[3:10].any() and bool((points[10:] != 0).any(axis=1).all())
        # a span shorter than its cloud: truncated
        points, counts = _pack_and_compare(r, C, [n[257], n[2]], [0, 100, 102], 110, kind, "short span")
        assert counts.tolist() == [257, 2] and bool((points[:102] != 0).any(axis=1).all()) and not points[102:].any()


@pytest.mark.parametrize("C", [8, 7, 3])
def test_pack_rows_in_front_of_the_first_sample_are_zeros(C):
    """out_first[0] = 5: the rows 0 .. 4 belong to no sample (their position inside sample 0's cloud is negative).  The
    cloud of sample 0 has more than 5 resident rows in front of it, so a kernel that gathered from the negative position
    would read inside the table and fail here by wrong values."""
    r = _resident(C)
    n = r["names"]
    assert int(r["first"][n[256]]) >= 5
    for kind in ("flips", "rotation"):
        points, counts = _pack_and_compare(r, C, [n[256], n[2]], [5, 261, 263], 300, kind, "out_first[0] = 5")
        assert counts.tolist() == [256, 2] and not points[:5].any() and bool((points[5:263] != 0).any(axis=1).all())


# ---------------------------------------------------------------------------------------------------------------------
# 4. targets
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _resident_wireframes():
    wfs, names = K.wireframes()
    wfv, wfe, vfirst, efirst = K.resident_wireframes(wfs)
    assert sorted({w[0].shape[0] for w in wfs}) == [0, 1, 2, 3, 16, 17, 300] and wfs[names["c300"]][1].shape[0] == 600
    return dict(wfs=wfs, names=names, host=(wfv, wfe, vfirst, efirst), dev=tuple(_to_dev(a) for a in (wfv, wfe, vfirst, efirst)))


def _target_batch(w, V):
    """every wireframe of at most V vertices, the smallest one above V where the issue asks for the clamp (V = 16 with
    c = 17; also V = 1 and V = 2), a repeat, and two cloud indices outside the resident wireframes"""
    wfs = w["wfs"]
    cloud = [i for i, (v, _) in enumerate(wfs) if v.shape[0] <= V]
    above = [i for i, (v, _) in enumerate(wfs) if v.shape[0] > V]
    if above and V != 300:
        cloud.append(min(reversed(above), key=lambda i: wfs[i][0].shape[0]))
    return cloud[:2] + [-1] + cloud[2:] + [len(wfs), cloud[-1]]


@pytest.mark.parametrize("kind", AUG_KINDS)
@pytest.mark.parametrize("V", [1, 2, 16, 300])
def test_wireframe_targets_every_edge_list(V, kind):
    w = _resident_wireframes()
    cloud = _target_batch(w, V)
    B, W = len(cloud), V * (V - 1) // 2
    if V == 16:
        assert w["names"]["c17"] in cloud
    aug = K.augmentation(kind, B, seed=V)
    block = _block(aug, cloud, np.zeros(B + 1, dtype=np.int32))          # out_first is not read by this kernel
    verts, exist = Guarded((B, V, 3), torch.float32), Guarded((B, V), torch.float32)
    counts, labels = Guarded((B,), torch.int64), Guarded((B, W), torch.float32)
    d_wfv, d_wfe, d_vfirst, d_efirst = w["dev"]
    _check(_lib().wf3d_wireframe_targets(d_wfv.data_ptr(), d_wfe.data_ptr(), d_vfirst.data_ptr(), d_efirst.data_ptr(), len(w["wfs"]),
                                         block.data_ptr(), B, V, verts.ptr(), exist.ptr(), counts.ptr(),
                                         None if V == 1 else labels.ptr(), _stream()), "wireframe_targets")
    want = M.targets_model(*w["host"], cloud, aug, V)
    g_counts, g_exist, g_labels = counts.read(), exist.read(), labels.read()
    assert np.array_equal(g_counts, want["vertex_counts"]) and np.array_equal(_bits(g_exist), _bits(want["vertex_existence"]))
    assert np.array_equal(_bits(g_labels), _bits(want["edge_labels"]))
    g_verts = verts.read()
    worst = _check_rows(g_verts, want["vertices"], kind == "rotation", (V, kind))
    for b, c in enumerate(want["vertex_counts"].tolist()):
        assert not _bits(g_verts[b, min(c, V):]).any()                  # +0.0 behind the vertices
    print(f"targets V={V} {kind}: {B} samples, {int(want['edge_labels'].sum())} labels set, x, y within {worst:.2f} float32 spacings")
