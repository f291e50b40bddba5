"""The augmentation extension on the GPU — wf3d_cloud_sample_dev_ext, wf3d_cloud_sample_fps_ext, wf3d_wireframe_targets_ext,
wf3d_cloud_epoch_params_ext and their way up through DeviceCloudCache — against wf3d/sampling.py, bit for bit.

The specification of a point: the source row idx(b, p_eff) (choice_indices or fps_indices at p_eff = effective_rows), the
plain form's float64 (xr, yr, z) — x = fx u0, y = fy u1, xr = fma(x, c, -(y s)), yr = fma(x, s, y c): the operations the
gather is written in, restated here with exact rational arithmetic and one rounding per fma — then
sampling.augment_point under the sample's extension row and sampling.jitter_noise.  Every comparison is of int32 views.

Shapes: resident clouds of 1, 5, 63, 64, 65 and 300 rows; P in {1, 7, 64, 130} (P > n: with replacement; P <= n: the
Feistel walk; wave and block tails); C in {8, 3, 7} (both gather kernels); B = 4 with one dead sample; extension rows mixing
identity, isotropic and anisotropic scale, a jitter whose clip binds (sigma = 1, clip = 0.5), drop = 0, 1 and 0.5."""
import functools
import os
import types
from fractions import Fraction

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from wf3d import sampling as S  # noqa: E402

ROWS = (1, 5, 63, 64, 65, 300)
PS = [1, 7, 64, 130]
CS = [8, 3, 7]
INF = float("inf")
# two batches of B = 4 over the six clouds, one dead sample each (a cloud index outside the resident clouds)
BATCHES = (
    ([0, 3, -1, 5], [(1, 1, 1, 0, INF, 0),                        # identity
                     (0.8, 1.1, 1.25, 1.0, 0.5, 0.5),             # anisotropic, a clip that binds, drop = 0.5
                     (1.3, 1.3, 1.3, 1.0, 0.5, 1.0),              # the dead sample: zeros whatever its row says
                     (1.2, 1.2, 1.2, 0.01, INF, 1.0)]),           # isotropic, unclipped jitter, drop = 1
    ([1, 2, 4, len(ROWS)], [(0.8, 0.8, 0.8, 0, INF, 0.0),         # isotropic, drop = 0
                            (1, 1, 1, 1.0, 0.5, 0),               # the binding clip alone
                            (1.25, 0.9, 1.0, 0, INF, 0.5),        # anisotropic without jitter, drop = 0.5
                            (1, 1, 1, 0, INF, 0)]),
)
WORD0 = 0x5EED1234
COLUMNS = {8: dict(use_color=True, use_intensity=True), 3: dict(use_color=False, use_intensity=False)}
TARGET_KEYS = ("vertices", "vertex_existence", "edge_labels", "vertex_counts")
CFG = {"scale": (0.8, 1.25), "anisotropic": True, "jitter_sigma": 0.02, "jitter_clip": 0.03, "max_dropout": 0.875}


def dev():
    return torch.device("cuda:0")


def _lib():
    from wf3d import _lib as L
    return L, L.load()


def _stream():
    from wf3d.ops import _stream as s
    return s()


def _bits(t):
    t = t.detach().cpu().contiguous() if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t))
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same_bits(a, b):
    a, b = _bits(a), _bits(b)
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


def _ext_rows(rows):
    return np.array([tuple(r) + (0.0, 0.0) for r in rows], dtype=np.float64)


# ---------------------------------------------------------------------------------------------------------------------
# the plain form's float64 values, restated
# ---------------------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    """fma(a, b, c) of finite float64: the exact a b + c, rounded once (float(Fraction) rounds to nearest even)"""
    exact = Fraction(a) * Fraction(b) + Fraction(c)
    return a * b + c if exact == 0 else float(exact)              # an exact zero: the sum of the (exact) parts has its sign


def rotated(aug_b, u0, u1):
    fx, fy, c, s = (float(v) for v in aug_b)
    x, y = fx * float(u0), fy * float(u1)
    return _fma(x, c, -(y * s)), _fma(x, s, y * c)


def spec_points(norm, first, cloud, aug, ext, word0, P, sampler):
    """(points float32 [B, P, C], idx int32 [B, P]) of the `_ext` samplers from host copies of everything they read"""
    C, B, ncl = norm.shape[1], len(cloud), len(first) - 1
    out, taken = np.zeros((B, P, C), dtype=np.float32), np.zeros((B, P), dtype=np.int32)
    for b, cl in enumerate(cloud):
        n = int(first[cl + 1] - first[cl]) if 0 <= cl < ncl else 0
        if n < 1:
            continue                                               # a dead sample: zeros
        rows = norm[int(first[cl]):int(first[cl]) + n]
        idx = S.choice_indices(word0, b, n, P) if sampler == "device" else S.fps_indices(word0, b, rows[:, :3], P)
        p_eff = S.effective_rows(word0, b, P, ext[b, 5])
        idx = idx[p_eff]
        taken[b] = idx
        noise = S.jitter_noise(word0, b, p_eff)
        xyz = np.array([rotated(aug[b], r[0], r[1]) + (r[2],) for r in rows[idx]], dtype=np.float64).reshape(P, 3)
        out[b, :, :3] = S.augment_point(xyz, ext[b], noise)
        out[b, :, 3:] = rows[idx, 3:].astype(np.float32)
    return out, taken


def spec_vertices(wfv, vfirst, cloud, aug, ext, V):
    B, ncl = len(cloud), len(vfirst) - 1
    out = np.zeros((B, V, 3), dtype=np.float32)
    for b, cl in enumerate(cloud):
        if not 0 <= cl < ncl:
            continue
        v = wfv[int(vfirst[cl]):int(vfirst[cl + 1])][:V]
        for i, r in enumerate(v):
            xr, yr = rotated(aug[b], r[0], r[1])
            out[b, i] = S.augment_point(np.array([xr, yr, r[2]]), (ext[b, 0], ext[b, 1], ext[b, 2], 0.0, INF, 0.0), np.zeros(3))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# a resident table made by hand: the entry points themselves
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _table(C):
    """clouds of ROWS rows x C columns (float64, unit-cube coordinates with a -0.0 and an exact 0), their row offsets, and
    a wireframe per cloud (0, 1, 4, 7, 2 and 8 vertices)"""
    rng = np.random.RandomState(100 + C)
    norm = rng.uniform(-1.0, 1.0, (sum(ROWS), C))
    norm[0, :3] = (-0.0, 0.0, -0.0)
    first = np.concatenate([[0], np.cumsum(ROWS)]).astype(np.int64)
    nv = (0, 1, 4, 7, 2, 8)
    wfv = rng.uniform(-1.0, 1.0, (sum(nv), 3))
    wfv[1] = (-0.0, 0.5, -0.0)
    vfirst = np.concatenate([[0], np.cumsum(nv)]).astype(np.int64)
    edges = [[(i, (i + 1) % c) for i in range(c)] if c > 1 else [] for c in nv]
    efirst = np.concatenate([[0], np.cumsum([len(e) for e in edges])]).astype(np.int64)
    wfe = np.array([p for e in edges for p in e], dtype=np.int32).reshape(-1, 2)
    host = dict(norm=norm, first=first, wfv=wfv, vfirst=vfirst, wfe=wfe, efirst=efirst)
    return host, {k: torch.from_numpy(v).to(dev()) for k, v in host.items()}


def _block(cloud, P, seed):
    """a parameter block of B samples with flips and a rotation each: (uint8 tensor on the device, aug [B, 4])"""
    rng = np.random.RandomState(seed)
    B = len(cloud)
    ang = rng.uniform(-np.pi / 36, np.pi / 36, B)
    aug = np.stack([rng.choice([-1.0, 1.0], B), rng.choice([-1.0, 1.0], B), np.cos(ang), np.sin(ang)], axis=1)
    raw = np.zeros(40 * B + 4, dtype=np.uint8)
    raw[:32 * B].view(np.float64)[:] = aug.reshape(-1)
    raw[32 * B:36 * B].view(np.int32)[:] = cloud
    raw[36 * B:].view(np.int32)[:] = np.arange(B + 1) * P
    return torch.from_numpy(raw).to(dev()), aug


def _run_sampler(sampler, d, block, words, B, P, C, ext=None):
    """(points, idx or None) of the plain (ext is None) or `_ext` entry point into poisoned outputs"""
    L, lib = _lib()
    pts = torch.full((B, P, C), 7.0, dtype=torch.float32, device=dev())
    more = () if ext is None else (ext.data_ptr(),)
    if sampler == "device":
        fn = lib.wf3d_cloud_sample_dev if ext is None else lib.wf3d_cloud_sample_dev_ext
        L.check(fn(d["norm"].data_ptr(), d["first"].data_ptr(), len(ROWS), block.data_ptr(), words.data_ptr(), B, P, C,
                   pts.data_ptr(), *more, _stream()), "cloud_sample_dev")
        return pts, None
    idx = torch.full((B, P), -7, dtype=torch.int32, device=dev())
    fn = lib.wf3d_cloud_sample_fps if ext is None else lib.wf3d_cloud_sample_fps_ext
    L.check(fn(d["norm"].data_ptr(), d["first"].data_ptr(), len(ROWS), block.data_ptr(), words.data_ptr(), B, P, C, pts.data_ptr(),
               idx.data_ptr(), max(ROWS), None, 0, *more, _stream()), "cloud_sample_fps")
    return pts, idx


# 1 and 2: both samplers are the specification; an identity block gives the plain entry point's bits
@pytest.mark.parametrize("sampler", ["device", "fps"])
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("P", PS)
def test_ext_samplers_are_the_specification(P, C, sampler):
    host, d = _table(C)
    words = torch.tensor([WORD0 - (1 << 32) if WORD0 >= 1 << 31 else WORD0, 0, 0, 0, 0], dtype=torch.int32, device=dev())
    for k, (cloud, rows) in enumerate(BATCHES):
        B = len(cloud)
        block, aug = _block(cloud, P, 10 * P + C + k)
        ext = _ext_rows(rows)
        pts, idx = _run_sampler(sampler, d, block, words, B, P, C, torch.from_numpy(ext).to(dev()))
        want, want_idx = spec_points(host["norm"], host["first"], cloud, aug, ext, WORD0, P, sampler)
        dead = [b for b, cl in enumerate(cloud) if not 0 <= cl < len(ROWS)]
        assert len(dead) == 1 and not want[dead[0]].any()
        assert _same_bits(pts, want)
        if idx is not None:
            assert _same_bits(idx, want_idx)
        # what the rows say: drop = 1 leaves copies of row 0, the binding clip is reached on both sides
        for b, row in enumerate(rows):
            if b in dead or P < 2:
                continue
            if row[5] == 1.0:
                assert bool((pts[b] == pts[b, 0]).all())
            if row[5] == 0.0 and sampler == "device" and P <= ROWS[cloud[b]] and row[3] == 0:
                assert len({tuple(r) for r in pts[b].cpu().numpy().tolist()}) == P      # distinct rows stay distinct
        # the identity block: the plain entry point's bits
        ident = torch.tensor(S.EXT_IDENTITY, dtype=torch.float64).repeat(B, 1).to(dev())
        got_i, idx_i = _run_sampler(sampler, d, block, words, B, P, C, ident)
        plain, idx_p = _run_sampler(sampler, d, block, words, B, P, C)
        assert _same_bits(got_i, plain) and (idx_i is None or torch.equal(idx_i, idx_p))
        assert P * C < 24 or not torch.equal(plain, pts)


def test_a_block_the_host_did_not_build_gives_nans_not_reads():
    """NaN scale, sigma and clip: NaN coordinates in that sample's x, y, z, the other columns and samples as specified"""
    C, P = 8, 64
    host, d = _table(C)
    words = torch.tensor([WORD0, 0, 0, 0, 0], dtype=torch.int32, device=dev())
    cloud = [5, 4, 3, 2]
    block, aug = _block(cloud, P, 5)
    nan = float("nan")
    ext = _ext_rows([(nan, 1, 1, 0, INF, 0), (1, 1, 1, nan, INF, 0), (1, 1, 1, 0.5, nan, 0), (1, 1, 1, 0, INF, nan)])
    pts, _ = _run_sampler("device", d, block, words, 4, P, C, torch.from_numpy(ext).to(dev()))
    plain, _ = _run_sampler("device", d, block, words, 4, P, C)
    assert bool(torch.isnan(pts[0, :, 0]).all()) and _same_bits(pts[0, :, 1:], plain[0, :, 1:])
    assert bool(torch.isnan(pts[1, :, :3]).all()) and bool(torch.isnan(pts[2, :, :3]).all())
    assert _same_bits(pts[1:3, :, 3:], plain[1:3, :, 3:])
    assert _same_bits(pts[3], plain[3])                            # a NaN drop drops nothing
    want, _ = spec_points(host["norm"], host["first"], cloud, aug, ext, WORD0, P, "device")
    assert np.array_equal(np.isnan(want), torch.isnan(pts).cpu().numpy())


# 3: the targets
@pytest.mark.parametrize("V", [1, 8])
def test_targets_ext_scales_the_vertices_only(V):
    L, lib = _lib()
    host, d = _table(8)
    for k, (cloud, rows) in enumerate(BATCHES):
        B = len(cloud)
        if V < 8:
            cloud = [cl if cl < 2 else 1 for cl in cloud]          # wireframes that fit V = 1
        block, aug = _block(cloud, 7, 50 + k)
        ext = _ext_rows(rows)

        def run(ext_dev):
            W = V * (V - 1) // 2
            out = {"vertices": torch.full((B, V, 3), 7.0, device=dev()), "vertex_existence": torch.full((B, V), 7.0, device=dev()),
                   "vertex_counts": torch.full((B,), -7, dtype=torch.int64, device=dev()),
                   "edge_labels": torch.full((B, W), 7.0, device=dev())}
            fn = lib.wf3d_wireframe_targets if ext_dev is None else lib.wf3d_wireframe_targets_ext
            L.check(fn(d["wfv"].data_ptr(), d["wfe"].data_ptr(), d["vfirst"].data_ptr(), d["efirst"].data_ptr(), len(ROWS), block.data_ptr(),
                       B, V, out["vertices"].data_ptr(), out["vertex_existence"].data_ptr(), out["vertex_counts"].data_ptr(),
                       out["edge_labels"].data_ptr() if W else None, *(() if ext_dev is None else (ext_dev.data_ptr(),)), _stream()),
                    "wireframe_targets")
            return out
        plain, got = run(None), run(torch.from_numpy(ext).to(dev()))
        assert _same_bits(got["vertices"], spec_vertices(host["wfv"], host["vfirst"], cloud, aug, ext, V))
        for key in ("vertex_existence", "vertex_counts", "edge_labels"):
            assert _same_bits(got[key], plain[key]), key
        ones = ext.copy()
        ones[:, :3] = 1.0                                          # sx = sy = sz = 1 (jitter and drop are not the targets')
        assert _same_bits(run(torch.from_numpy(ones).to(dev()))["vertices"], plain["vertices"])
        assert V == 1 or not torch.equal(got["vertices"], plain["vertices"])


# 4: the epoch kernel
def _epoch_call(state, members, first, B, world, rank, P, augment, cfg8=None):
    """(params uint8, words int32 [5], ext or None) of one call on `state` (advanced by it)"""
    L, lib = _lib()
    params = torch.full((40 * B + 4,), 249, dtype=torch.uint8, device=dev())
    words = torch.full((5,), -7, dtype=torch.int32, device=dev())
    ext = None if cfg8 is None else torch.full((B, 8), 7.0, dtype=torch.float64, device=dev())
    fn = lib.wf3d_cloud_epoch_params if cfg8 is None else lib.wf3d_cloud_epoch_params_ext
    more = () if cfg8 is None else (cfg8.ctypes.data, ext.data_ptr())
    code = fn(state.data_ptr(), members.data_ptr(), members.numel(), first.data_ptr(), len(ROWS), B, world, rank, P, augment,
              params.data_ptr(), words.data_ptr(), *more, _stream())
    return code, params, words, ext


def _i64(x):
    return x - (1 << 64) if x >= 1 << 63 else x


@pytest.mark.parametrize("cfg", [CFG, {"scale": (0.5, 2.0)}, {"jitter_sigma": 0.01, "max_dropout": 0.5}])
def test_epoch_params_ext_is_the_specification(cfg):
    _, d = _table(8)
    key, D, B, P = 0xC0FFEE1234567891, 23, 2, 7
    members_h = np.random.RandomState(4).randint(0, len(ROWS), D).astype(np.int32)
    members = torch.from_numpy(members_h).to(dev())
    cfg8 = S.augment_cfg8(cfg)
    for world, rank in ((1, 0), (2, 0), (2, 1)):
        steps = S.epoch_steps(D, B, world, rank)
        for t0 in (0, steps - 2):                                  # t0 .. t0 + 3: across an epoch boundary from steps - 2
            state = torch.tensor([_i64(key), t0], dtype=torch.int64, device=dev())
            for t in range(t0, t0 + 4):
                twin = state.clone()
                code, params, words, ext = _epoch_call(state, members, d["first"], B, world, rank, P, 1, cfg8)
                assert code == 0
                assert state.tolist() == [_i64(key), t + 1]        # one step per call
                spec = S.epoch_batch(key, t, D, B, world, rank, True, augment_ext=cfg)
                assert np.array_equal(ext.cpu().numpy().view(np.int64), spec["ext"].view(np.int64))
                assert np.array_equal(words.cpu().numpy().view(np.uint32), spec["seed_words"])
                raw = params.cpu().numpy()
                assert np.array_equal(raw[:32 * B].view(np.int64), spec["aug"].reshape(-1).view(np.int64))
                assert raw[32 * B:36 * B].view(np.int32).tolist() == members_h[spec["order"]].tolist()
                assert raw[36 * B:].view(np.int32).tolist() == [b * P for b in range(B + 1)]
                code, params_p, words_p, _ = _epoch_call(twin, members, d["first"], B, world, rank, P, 1)
                assert code == 0 and torch.equal(params, params_p) and torch.equal(words, words_p) and torch.equal(twin, state)
    # the packed form's block (P = 0) and no flips: still the plain entry point's
    state = torch.tensor([_i64(key), 5], dtype=torch.int64, device=dev())
    twin = state.clone()
    _, params, _, ext = _epoch_call(state, members, d["first"], B, 1, 0, 0, 0, cfg8)
    assert torch.equal(params, _epoch_call(twin, members, d["first"], B, 1, 0, 0, 0)[1])
    assert np.array_equal(ext.cpu().numpy(), S.epoch_batch(key, 5, D, B, augment=False, augment_ext=cfg)["ext"])


# 7: refusals, before any launch
def test_argument_checks_launch_nothing():
    L, lib = _lib()
    ERR = L.DEFINES["WF3D_ERR_ARG"]
    _, d = _table(8)
    B, P, C, V = 2, 7, 8, 8
    block, _ = _block([5, 4], P, 1)
    words = torch.zeros(5, dtype=torch.int32, device=dev())
    pts = torch.full((B, P, C), 7.0, device=dev())
    idx = torch.full((B, P), -7, dtype=torch.int32, device=dev())
    ext = torch.tensor(S.EXT_IDENTITY, dtype=torch.float64).repeat(B, 1).to(dev())
    for bad in (None, ext.data_ptr() + 4):                         # NULL, misaligned
        assert lib.wf3d_cloud_sample_dev_ext(d["norm"].data_ptr(), d["first"].data_ptr(), len(ROWS), block.data_ptr(), words.data_ptr(),
                                             B, P, C, pts.data_ptr(), bad, None) == ERR
        assert b"wf3d_cloud_sample_dev_ext" in lib.wf3d_last_error()
        assert lib.wf3d_cloud_sample_fps_ext(d["norm"].data_ptr(), d["first"].data_ptr(), len(ROWS), block.data_ptr(), words.data_ptr(),
                                             B, P, C, pts.data_ptr(), idx.data_ptr(), max(ROWS), None, 0, bad, None) == ERR
        assert b"wf3d_cloud_sample_fps_ext" in lib.wf3d_last_error()
        tv, te, tc = torch.full((B, V, 3), 7.0, device=dev()), torch.full((B, V), 7.0, device=dev()), torch.full((B,), -7, dtype=torch.int64, device=dev())
        tl = torch.full((B, V * (V - 1) // 2), 7.0, device=dev())
        assert lib.wf3d_wireframe_targets_ext(d["wfv"].data_ptr(), d["wfe"].data_ptr(), d["vfirst"].data_ptr(), d["efirst"].data_ptr(),
                                              len(ROWS), block.data_ptr(), B, V, tv.data_ptr(), te.data_ptr(), tc.data_ptr(), tl.data_ptr(),
                                              bad, None) == ERR
        assert b"wf3d_wireframe_targets_ext" in lib.wf3d_last_error()
        torch.cuda.synchronize()
        assert bool((pts == 7.0).all()) and bool((idx == -7).all()) and bool((tv == 7.0).all()) and bool((tc == -7).all())
    # the plain checks still come first in the `_ext` forms
    assert lib.wf3d_cloud_sample_dev_ext(d["norm"].data_ptr(), d["first"].data_ptr(), len(ROWS), block.data_ptr(), words.data_ptr(),
                                         0, P, C, pts.data_ptr(), ext.data_ptr(), None) == ERR
    # every entry of cfg
    members = torch.arange(6, dtype=torch.int32, device=dev())
    good = S.augment_cfg8(CFG)
    nan = float("nan")
    bads = [(0, 0.0), (0, -1.0), (0, nan), (0, 2.0), (1, INF), (1, nan), (2, 0.5), (2, nan), (3, -0.1), (3, INF), (3, nan),
            (4, 0.0), (4, -1.0), (4, nan), (5, -0.1), (5, 1.5), (5, nan), (6, 1.0), (7, 1.0)]
    for k, value in bads:
        cfg8 = good.copy()
        cfg8[k] = value
        state = torch.tensor([1, 3], dtype=torch.int64, device=dev())
        code, params, w, e = _epoch_call(state, members, d["first"], B, 1, 0, P, 1, cfg8)
        assert code == ERR and b"wf3d_cloud_epoch_params_ext" in lib.wf3d_last_error(), (k, value)
        torch.cuda.synchronize()
        assert state.tolist() == [1, 3] and bool((params == 249).all()) and bool((e == 7.0).all()) and bool((w == -7).all())
    state = torch.tensor([1, 3], dtype=torch.int64, device=dev())
    L2 = lib.wf3d_cloud_epoch_params_ext
    params = torch.zeros(40 * B + 4, dtype=torch.uint8, device=dev())
    args = (state.data_ptr(), members.data_ptr(), 6, d["first"].data_ptr(), len(ROWS), B, 1, 0, P, 1, params.data_ptr(), words.data_ptr())
    assert L2(*args, None, ext.data_ptr(), None) == ERR and L2(*args, good.ctypes.data, None, None) == ERR
    assert L2(*args, good.ctypes.data, ext.data_ptr() + 4, None) == ERR
    good_inf = good.copy()
    good_inf[4] = INF                                              # an infinite clip is no error
    assert L2(*args, good_inf.ctypes.data, ext.data_ptr(), None) == 0 and state.tolist() == [1, 4]


# ---------------------------------------------------------------------------------------------------------------------
# through DeviceCloudCache: a tiny data set on disk
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_root(tmp_path_factory):
    """<root>/train/{xyz, wireframe}: clouds of ROWS rows x 8 columns, each with a 4-vertex wireframe"""
    from datasets.building3d import save_wireframe
    root = tmp_path_factory.mktemp("tiny_augment")
    os.makedirs(root / "train" / "xyz")
    os.makedirs(root / "train" / "wireframe")
    rng = np.random.RandomState(12)
    for k, rows in enumerate(ROWS):
        cloud = np.concatenate([rng.uniform(-1.0, 1.0, (rows, 3)), rng.randint(0, 256, (rows, 4)).astype(np.float64),
                                rng.uniform(0.0, 1.0, (rows, 1))], axis=1)
        np.savetxt(root / "train" / "xyz" / f"{k + 1}.xyz", cloud, fmt="%.17g")
        save_wireframe(rng.uniform(-1.0, 1.0, (4, 3)), [(0, 1), (1, 2), (2, 3), (0, 3)], str(root / "train" / "wireframe" / f"{k + 1}.obj"))
    return str(root)


@functools.lru_cache(maxsize=None)
def _pair(root, P, C, augment):
    from datasets import Building3DReconstructionDataset, DeviceCloudCache
    cfg = types.SimpleNamespace(root_dir=root, num_points=P, normalize=False, augment=augment, **COLUMNS[C])
    ds = Building3DReconstructionDataset(cfg, split_set="train")
    torch.manual_seed(77 * P + C + augment)
    cache = DeviceCloudCache(ds, dev())
    host = dict(norm=cache.norm.cpu().numpy(), first=cache.first.cpu().numpy(), wfv=cache.wf_vertices.cpu().numpy(),
                vfirst=cache.vfirst.cpu().numpy())
    return ds, cache, host


def _check_filled(buf, host, cloud, aug, ext, word0, sampler):
    B, P, V = buf["points"].shape[0], buf["points"].shape[1], buf["vertices"].shape[1]
    want, want_idx = spec_points(host["norm"], host["first"], cloud, aug, ext, word0, P, sampler)
    assert _same_bits(buf["points"], want)
    if sampler == "fps":
        assert _same_bits(buf["point_indices"], want_idx)
    assert _same_bits(buf["vertices"], spec_vertices(host["wfv"], host["vfirst"], cloud, aug, ext, V))


# 5: one capture, three replays, three batches of the specification
@pytest.mark.parametrize("sampler,C,P,augment", [("device", 8, 64, True), ("fps", 8, 7, True), ("device", 3, 130, False)])
def test_captured_fill_epoch_walks_the_specification(tiny_root, sampler, C, P, augment):
    ds, cache, host = _pair(tiny_root, P, C, augment)
    B, V = 2, 4
    buf = cache.sampled_buffers(B, V, sampler=sampler, augment=CFG)
    assert buf["augment"] == S.check_augment(CFG) and tuple(buf["aug_ext"].shape) == (B, 8) and buf["aug_ext"].dtype == torch.float64
    assert buf["aug_ext"].is_cuda and buf["aug_ext_host"].is_pinned()
    assert buf["aug_ext"].cpu().tolist() == [list(S.EXT_IDENTITY)] * B
    smp = cache.epoch_sampler(B, seed=0xABCDEF)
    assert smp.steps_per_epoch == 3
    cache.fill_epoch(buf, smp)                                     # eager once: batch 0
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cache.fill_epoch(buf, smp)
    smp.seek(0, 2)                                                 # the replays: batches 2, 3 and 4, over the epoch's end
    shots = []
    for t in (2, 3, 4):
        graph.replay()
        torch.cuda.synchronize()
        spec = smp.batch_at(t, augment_ext=CFG)
        block, ext = smp.block_at(t, P, augment_ext=CFG)
        assert torch.equal(buf["params"].cpu(), block) and _same_bits(buf["aug_ext"].cpu().view(torch.int64), ext.view(torch.int64))
        word0 = int(spec["seed_words"][0])
        assert (int(buf["sample_words"][0]) & 0xFFFFFFFF) == word0
        _check_filled(buf, host, spec["cloud"].tolist(), spec["aug"], spec["ext"], word0, sampler)
        shots.append((spec["cloud"].tolist(), buf["points"].clone()))
    assert int(smp.get_state()[1]) == 5
    # the jitter differs between replays: the same cloud in two batches never gives the same points
    assert not torch.equal(shots[0][1], shots[1][1]) and not torch.equal(shots[1][1], shots[2][1])
    # without flips and rotation the extension still applies, and plain buffers are untouched by it
    plain = cache.sampled_buffers(B, V, sampler=sampler)
    assert "aug_ext" not in plain and "augment" not in plain and "aug_ext" not in cache.sampled_buffers(B, V, sampler=sampler, augment={})


# 6: the host-staged forms
@pytest.mark.parametrize("sampler,C,P,cfg", [("device", 8, 64, CFG), ("fps", 3, 7, CFG), ("device", 8, 130, {"scale": (0.9, 1.1)}),
                                            ("device", 3, 64, {"jitter_sigma": 0.01, "max_dropout": 0.5})])
def test_stage_fill_and_batch_follow_the_host_draws(tiny_root, sampler, C, P, cfg):
    from datasets.building3d import rotz
    ds, cache, host = _pair(tiny_root, P, C, True)
    idxs = [5, 0, 3, 4]
    B, V = len(idxs), 4
    n_scale, n_drop = S.ext_draws(cfg)

    def host_draws(seed):
        """the documented consumption: the batch's flips and angles, then per sample the scale value(s) and the ratio"""
        np.random.seed(seed)
        draws = [ds._draw_augmentation() for _ in range(B)]
        aug = np.array([(fx, fy, np.cos(t), np.sin(t)) for fx, fy, t in draws])
        ext = np.stack([S.ext_row(cfg, [np.random.random() for _ in range(n_scale)], np.random.random() if n_drop else None)
                        for _ in range(B)])
        return draws, aug, ext, np.random.random()

    buf = cache.sampled_buffers(B, V, sampler=sampler, augment=cfg)
    np.random.seed(61)
    cache.stage(buf, idxs)
    after = np.random.random()
    cache.fill(buf)
    torch.cuda.synchronize()
    draws, aug, ext, want_after = host_draws(61)
    assert after == want_after
    assert np.array_equal(buf["aug_ext_host"].numpy(), ext) and torch.equal(buf["aug_ext"].cpu(), buf["aug_ext_host"])
    assert np.array_equal(cache._block_views(buf["params_host"], B)[0], aug)
    _check_filled(buf, host, idxs, aug, ext, int(buf["sample_words"][0]) & 0xFFFFFFFF, sampler)
    # plain buffers under the same seed: the same flips and angles, and np.random left where it was before the extension's draws
    plain = cache.sampled_buffers(B, V, sampler=sampler)
    np.random.seed(61)
    cache.stage(plain, idxs)
    after_plain = np.random.random()
    np.random.seed(61)
    for _ in range(B):
        ds._draw_augmentation()
    assert np.random.random() == after_plain
    assert torch.equal(plain["params_host"], buf["params_host"])
    # batch(..., augment=)
    np.random.seed(62)
    got = cache.batch(idxs, sampler=sampler, augment=cfg)
    after = np.random.random()
    draws, aug, ext, want_after = host_draws(62)
    assert after == want_after and np.array_equal(got["aug_ext"].cpu().numpy(), ext)
    want_pts, want_idx = spec_points(host["norm"], host["first"], idxs, aug, ext, int(cache.last_sample_words[0]) & 0xFFFFFFFF, P, sampler)
    assert _same_bits(got["point_clouds"], want_pts)
    if sampler == "fps":
        assert _same_bits(got["point_indices"], want_idx)
    items = ds.collate_batch([cache._item(i, fx, fy, rotz(t), ext[b, :3]) for b, (i, (fx, fy, t)) in enumerate(zip(idxs, draws))])
    unscaled = ds.collate_batch([cache._item(i, fx, fy, rotz(t)) for i, (fx, fy, t) in zip(idxs, draws)])
    for key in ("wf_vertices", "wf_centers", "wf_edges_vertices"):
        assert all(torch.equal(a, b) for a, b in zip(got[key], items[key])), key
    for b in range(B):
        scale = torch.from_numpy(ext[b, :3])
        assert torch.allclose(got["wf_vertices"][b].double(), unscaled["wf_vertices"][b].double() * scale, rtol=1e-6, atol=1e-7)


def test_refusals_name_the_limit(tiny_root):
    ds, cache, _ = _pair(tiny_root, 64, 8, True)
    cfg = {"scale": (0.9, 1.1)}
    with pytest.raises(ValueError, match="fixed-size sampled batches only"):
        cache.packed_buffers(2, 1024, 4, augment=cfg)
    with pytest.raises(ValueError, match="fixed-size sampled batches only"):
        cache.packed_batch([0, 1], augment=cfg)
    with pytest.raises(ValueError, match="augment= needs sampler='device' or 'fps'"):
        cache.batch([0, 1], augment=cfg)
    with pytest.raises(ValueError, match="augment= needs sampler='device' or 'fps'"):
        cache.batch([0, 1], sampler="numpy", augment=cfg)
    with pytest.raises(ValueError, match="max_dropout must be in"):
        cache.sampled_buffers(2, 4, augment={"max_dropout": 2.0})
    # None and {} are no extension: the calls go through as before
    np.random.seed(1)
    a = cache.batch([0, 1], augment=None)["point_clouds"]
    np.random.seed(1)
    assert torch.equal(a, cache.batch([0, 1], augment={})["point_clouds"])
    assert "aug_ext" not in cache.packed_buffers(2, 1024, 4, augment=None)
