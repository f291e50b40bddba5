"""Drop-in `datasets.building3d` (reference datasets/building3d.py:18-202) — row f-3, the input pipeline in
front of the hot path — plus its MI355X form, `DeviceCloudCache`.

`Building3DReconstructionDataset` keeps the reference's constructor, `__getitem__` dict (same keys, dtypes, values),
`collate_batch` and `load_files`, so `main.py` / `evaluate.py` / a torch DataLoader work unchanged; it draws from
`np.random` in the reference's order (sampling choice, then flip-x, flip-y, angle), so a seeded run reproduces the
reference's samples.  The .xyz text is read by the library's C parser instead of `np.loadtxt` (~30x faster).

`DeviceCloudCache(dataset, device)` is the resident form: every cloud is parsed once, uploaded as float64 (the raw
coordinates are UTM metres — fp32 cannot hold them), normalised once on the device (csrc/cloud.hip) and kept in HBM;
`cache.batch(indices)` then costs one small host->device copy of the random choices and ONE gather/augment kernel that
writes the model's `[B, num_points, C]` fp32 input directly — no per-sample file I/O, no per-sample host arrays.

The packed form (whole clouds, `forward_packed`): `cache.packed_batch(indices)` is `collate_packed` of the same data set
with `num_points = 0`; `cache.packed_buffers` / `stage` / `fill` feed the static buffers of a captured step — `stage`
draws the augmentation and copies one 40·B + 4 byte parameter block, `fill` is two launches (points + point counts,
training targets) that read everything else from resident device memory.  `packed_plan` is the host part on its own.

The fixed-size form without per-point host data: `cache.sampled_buffers` / `stage` / `fill` do the same for
`[B, num_points, C]` batches whose rows are chosen IN the kernel (wf3d/sampling.py states the index function) under a seed
word that `fill` draws on the device, so one captured step trains as the reference trains — random fixed-size subsets,
flips, z-rotation; `cache.batch(indices, sampler="device")` is the same sampler for one batch.  `sampler="fps"` in either
chooses the rows by farthest-point sampling instead (wf3d/sampling.py `fps_indices`), in the same launches.

Resident epochs: `cache.epoch_sampler` / `fill_epoch` replace `stage` by a kernel — which clouds a batch holds (a keyed
permutation per epoch, sharded over ranks), the augmentation and the seed words come from a 16-byte state in device memory
(wf3d/sampling.py `epoch_batch` states them), so a loop of graph replays with nothing between them walks the data set.

The augmentation extension: `augment=cfg` (wf3d.sampling.check_augment: scale, anisotropic, jitter_sigma, jitter_clip,
max_dropout) on `sampled_buffers` or on `batch(..., sampler="device" | "fps")` adds a random scale, per-point jitter and
random point dropout INSIDE the same gather launch (wf3d/sampling.py `augment_point`), independent of the data set's
`augment` (flips and rotation).  The per-sample values live in an extension block of 64 B bytes beside the parameter
block; `stage` draws them from np.random, `fill_epoch` on the device."""
import ctypes
import glob
import operator
import os
from collections import defaultdict

import numpy as np
import torch
from torch.utils.data import Dataset

from wf3d._lib import DEFINES as _DEFINES


def _read_xyz(path, ncols=None):
    """[n, c] float64 rows of a whitespace-separated text file — what `np.loadtxt(path, dtype=np.float64)` returns
    (reference :98): the column count is the file's own (every row must have it; `ncols`, if given, is checked against
    it), `#` starts a comment.  Parsed by the library's C routine (wf3d_parse_table, ~30x faster than loadtxt); if
    libwf3d.so cannot be loaded at all — a host without ROCm preparing data — np.loadtxt does the same job."""
    try:
        from wf3d import _lib
        lib = _lib.load()
    except (OSError, ImportError):
        arr = np.atleast_2d(np.loadtxt(path, dtype=np.float64))
        if ncols is not None and arr.shape[1] != ncols:
            raise ValueError(f"{path}: {arr.shape[1]} columns, expected {ncols}")
        return arr
    cap = max(1024, os.path.getsize(path) // 4)
    cols = ctypes.c_long(0)
    buf = np.empty(cap, dtype=np.float64)
    n = lib.wf3d_parse_table(path.encode(), buf.ctypes.data_as(ctypes.c_void_p), cap, ctypes.byref(cols))
    if n > cap:
        buf = np.empty(n, dtype=np.float64)
        n = lib.wf3d_parse_table(path.encode(), buf.ctypes.data_as(ctypes.c_void_p), n, ctypes.byref(cols))
    if n == -3:
        raise ValueError(f"{path}: rows with different numbers of columns")
    if n < 0:
        raise OSError(f"cannot parse {path} (code {n})")
    c = int(cols.value)
    if ncols is not None and c != ncols and n:
        raise ValueError(f"{path}: {c} columns, expected {ncols}")
    return buf[:n].reshape(-1, c).copy() if n else np.empty((0, ncols or 0))


def load_wireframe(wireframe_file):
    """.obj wireframe: `v x y z` vertex lines, `l i j` (1-based) edge lines -> (vertices [n, 3] float64, edges [m, 2]).
    Edges are de-duplicated as sorted 0-based pairs through a set, in first-seen insertion order (reference :18-31)."""
    vertices, edges = [], set()
    with open(wireframe_file) as f:
        for raw in f.readlines():
            tok = raw.strip().split(" ")
            if tok[0] == "v":
                vertices.append(tok[1:])
            else:
                a, b = (np.array(tok[1:], dtype=np.int32).reshape(2) - 1).tolist()
                edges.add((a, b) if a <= b else (b, a))
    return np.array(vertices, dtype=np.float64), np.array(list(edges))


def save_wireframe(vertices, edges, wireframe_file):
    """Write an .obj that load_wireframe reads back: one `v x y z` line per vertex, one 1-based `l i j` line per edge."""
    lines = ["v " + " ".join(str(c) for c in v) for v in np.asarray(vertices)]
    lines += ["l " + " ".join(str(int(k) + 1) for k in e) for e in np.asarray(edges)]
    with open(wireframe_file, "w") as f:
        f.write("\n".join(lines) + "\n")


def random_sampling(pc, num_points, replace=None):
    """`num_points` random rows, with replacement iff the cloud is smaller (one np.random.choice draw, as reference :50-65)."""
    if replace is None:
        replace = pc.shape[0] < num_points
    return pc[np.random.choice(pc.shape[0], num_points, replace=replace)]


def rotz(t):
    """Rotation about the z-axis."""
    c, s = np.cos(t), np.sin(t)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])


def _columns(use_color, use_intensity):
    """(number of columns kept, [lo, hi) of the colour columns that are divided by 256) — reference :101-110."""
    if not use_color and not use_intensity:
        return 3, (0, 0)
    if use_color and not use_intensity:
        return 7, (3, 7)
    if use_color and use_intensity:
        return 8, (3, 7)
    # the reference concatenates a 2-D and a 1-D array here (:107) and numpy raises
    raise ValueError("use_color=False with use_intensity=True: all the input array dimensions except for the concatenation "
                     "axis must match exactly (the reference fails the same way, datasets/building3d.py:107)")


def _edge_vertices(wf_vertices, wf_edges):
    """[E, 2, 3] endpoints with the HIGHER-z vertex first (flip of an ascending argsort over z, reference :148-152),
    and the edge centres."""
    ev = np.stack((wf_vertices[wf_edges[:, 0]], wf_vertices[wf_edges[:, 1]]), axis=1)
    order = np.flip(np.argsort(ev[:, :, -1]), axis=1)
    ev = ev[np.arange(ev.shape[0])[:, np.newaxis], order]
    return ev, (ev[..., 0, :] + ev[..., 1, :]) / 2


class Building3DReconstructionDataset(Dataset):
    def __init__(self, dataset_config, split_set, logger=None):
        self.dataset_config = dataset_config
        self.roof_dir = dataset_config.root_dir
        self.num_points = dataset_config.num_points
        self.use_color = dataset_config.use_color
        self.use_intensity = dataset_config.use_intensity
        self.normalize = dataset_config.normalize
        self.augment = dataset_config.augment
        assert split_set in ["train", "test"]
        self.split_set = split_set
        self.pc_files, self.wireframe_files = self.load_files()
        if logger:
            logger.info("Total Sample: %d" % len(self.pc_files))

    def __len__(self):
        return len(self.pc_files)

    def _draw_augmentation(self):
        """(flip_x, flip_y, angle) from np.random in the reference's order (:131-141)."""
        fx = -1.0 if np.random.random() > 0.5 else 1.0
        fy = -1.0 if np.random.random() > 0.5 else 1.0
        return fx, fy, (np.random.random() * np.pi / 18) - np.pi / 36          # -5 .. +5 degrees

    def _finish(self, point_cloud, wf_vertices, wf_edges, centroid, max_distance, pc_file):
        ev, centers = _edge_vertices(wf_vertices, wf_edges)
        ret = {"point_clouds": point_cloud.astype(np.float32),
               "wf_vertices": wf_vertices.astype(np.float32),
               "wf_edges": wf_edges.astype(np.int64),
               "wf_centers": centers.astype(np.float32),
               "wf_edge_number": wf_edges.shape[0],
               "wf_edges_vertices": ev.reshape((-1, 6)).astype(np.float32)}
        if self.normalize:
            ret["centroid"] = centroid
            ret["max_distance"] = max_distance
        ret["scan_idx"] = np.array(os.path.splitext(os.path.basename(pc_file))[0]).astype(np.int64)
        return ret

    def __getitem__(self, index):
        pc_file = self.pc_files[index]
        pc = _read_xyz(pc_file)
        ncol, (clo, chi) = _columns(self.use_color, self.use_intensity)
        point_cloud = pc[:, :ncol]
        if chi > clo:
            point_cloud[:, clo:chi] = point_cloud[:, clo:chi] / 256.0
        wf_vertices, wf_edges = load_wireframe(self.wireframe_files[index])
        centroid = max_distance = None
        if self.normalize:
            centroid = np.mean(point_cloud[:, 0:3], axis=0)
            point_cloud[:, 0:3] -= centroid
            max_distance = np.max(np.linalg.norm(point_cloud[:, 0:3], axis=1))
            point_cloud[:, 0:3] /= max_distance
            wf_vertices -= centroid
            wf_vertices /= max_distance
        if self.num_points:
            point_cloud = random_sampling(point_cloud, self.num_points)
        if self.augment:
            fx, fy, angle = self._draw_augmentation()
            if fx < 0:
                point_cloud[:, 0] = -1 * point_cloud[:, 0]
                wf_vertices[:, 0] = -1 * wf_vertices[:, 0]
            if fy < 0:
                point_cloud[:, 1] = -1 * point_cloud[:, 1]
                wf_vertices[:, 1] = -1 * wf_vertices[:, 1]
            rt = np.transpose(rotz(angle))
            point_cloud[:, 0:3] = np.dot(point_cloud[:, 0:3], rt)
            wf_vertices[:, 0:3] = np.dot(wf_vertices[:, 0:3], rt)
        return self._finish(point_cloud, wf_vertices, wf_edges, centroid, max_distance, pc_file)

    @staticmethod
    def collate_batch(batch):
        """Variable-length wireframe entries stay lists of float32 tensors, everything else is stacked (reference :171-190)."""
        gathered = defaultdict(list)
        for item in batch:
            for key, val in item.items():
                gathered[key].append(val)
        out = {}
        for key, val in gathered.items():
            if key in ("wf_vertices", "wf_edges", "wf_centers", "wf_edges_vertices"):
                out[key] = [torch.from_numpy(v.astype(np.float32)) for v in val]
            else:
                out[key] = torch.tensor(np.array(val))
        return out

    @staticmethod
    def collate_packed(batch):
        """collate_batch for items whose point clouds differ in length (a dataset without num_points): `point_clouds` is the
        clouds concatenated along the point axis, [sum N_b, Din], and `point_counts` their lengths (int64 [B]) — the packed
        form of PointCloudToWireframe.forward_packed.  Every other field is as in collate_batch."""
        if not batch:
            raise ValueError("collate_packed: an empty batch")
        clouds = [np.asarray(item["point_clouds"]) for item in batch]
        rest = Building3DReconstructionDataset.collate_batch([{k: v for k, v in item.items() if k != "point_clouds"} for item in batch])
        rest["point_clouds"] = torch.from_numpy(np.ascontiguousarray(np.concatenate(clouds, axis=0)))
        rest["point_counts"] = torch.tensor([c.shape[0] for c in clouds], dtype=torch.int64)
        return rest

    def load_files(self):
        data_dir = os.path.join(self.roof_dir, self.split_set)
        pc_files = list(glob.glob(os.path.join(data_dir, "xyz", "*.xyz")))
        wf_files = [p.replace(os.path.sep + "xyz", os.path.sep + "wireframe").replace(".xyz", ".obj") for p in pc_files]
        return pc_files, wf_files


FPS_REG_ROWS = _DEFINES["WF3D_FPS_REG_ROWS"]      # farthest-point sampling keeps clouds up to this many rows in registers
SAMPLERS = ("numpy", "device", "fps")
PARAM_BYTES = 40       # per sample in the parameter block of a packed batch: aug 4 doubles, cloud int32, out_first int32


def packed_plan(n, vertex_counts, indices, draw=None, capacity=None, max_vertices=None, who="packed_plan", num_points=None):
    """The host part of a packed batch from resident clouds; needs no GPU.  `n` / `vertex_counts`: rows and wireframe
    vertices per resident cloud; `indices`: the batch (negative indices count from the end, as for a list); `draw`: the
    data set's `_draw_augmentation` when it augments, else None.  Returns (indices, out_first, aug): the normalised
    indices, int32 [B + 1] first output rows (out_first[B] = the batch's rows) and float64 [B, 4] {flip_x, flip_y, cos t,
    sin t} — the parameter block of include/wf3d.h.  np.random is consumed as `[ds0[i] for i in indices]` consumes it
    (ds0 = the data set with num_points = 0): per sample flip-x, flip-y, angle, and nothing without `draw`.  Every check
    comes before the first draw: IndexError for an index out of range, ValueError for an empty batch, for more than
    `capacity` rows and for a wireframe of more than `max_vertices` vertices.
    `num_points` = P: the plan of a FIXED-SIZE batch sampled on the device (wf3d_cloud_sample_dev) — out_first[b] = b * P,
    no row capacity (a cloud of any length fits; ValueError only for B * P >= 2^31), the same checks otherwise and the
    same draws in the same order."""
    indices = [operator.index(i) for i in indices]
    indices = [i + len(n) if i < 0 else i for i in indices]
    if any(not 0 <= i < len(n) for i in indices):
        raise IndexError(f"DeviceCloudCache.{who}: index out of range for {len(n)} clouds")
    if not indices:
        raise ValueError(f"DeviceCloudCache.{who}: an empty batch")
    if num_points is None:
        out_first = np.zeros(len(indices) + 1, dtype=np.int64)
        np.cumsum([n[i] for i in indices], out=out_first[1:])
        rows = int(out_first[-1])
        if rows > (0x7FFFFFFF if capacity is None else capacity):
            raise ValueError(f"DeviceCloudCache.{who}: the clouds hold {rows} points, above the capacity of {capacity} rows")
    else:
        P = operator.index(num_points)
        if P < 1 or len(indices) * P > 0x7FFFFFFF:
            raise ValueError(f"DeviceCloudCache.{who}: needs num_points >= 1 and B * num_points < 2^31 (got {len(indices)} x {P})")
        out_first = np.arange(len(indices) + 1, dtype=np.int64) * P
    most = max(vertex_counts[i] for i in indices)
    if max_vertices is not None and most > max_vertices:
        raise ValueError(f"a wireframe has {most} vertices, more than max_vertices = {max_vertices}")
    aug = np.empty((len(indices), 4), dtype=np.float64)
    for b in range(len(indices)):
        fx, fy, angle = draw() if draw is not None else (1.0, 1.0, 0.0)
        aug[b] = (fx, fy, np.cos(angle), np.sin(angle))
    return indices, out_first.astype(np.int32), aug


class DeviceCloudCache:
    """All clouds of a dataset resident in HBM, normalised once; batches are produced by one kernel.

        cache = DeviceCloudCache(dataset, torch.device("cuda:0"))
        batch = cache.batch([3, 0, 7])      # same dict as collate_batch([dataset[3], dataset[0], dataset[7]]), with
                                            # batch["point_clouds"] a device tensor; np.random is consumed identically

    Whole clouds for forward_packed (the data set's num_points is not used; a data set without one is accepted):

        batch = cache.packed_batch([3, 0, 7])          # collate_packed of the same data set with num_points = 0
        buf = cache.packed_buffers(B, capacity, max_vertices)      # static buffers of a captured step
        info = cache.stage(buf, [3, 0, 7])             # host: checks, np.random draws, one small non-blocking copy
        cache.fill(buf)                                # two launches; inside the capture, or before graph.replay()

    Fixed-size batches sampled on the device (another random stream than np.random.choice, the same distribution):

        batch = cache.batch([3, 0, 7], sampler="device")
        buf = cache.sampled_buffers(B, max_vertices)   # points [B, num_points, C]; stage / fill as above, three launches

    The same with the rows by farthest-point sampling (even coverage instead of the scanner's density; the seed word
    picks the start row): `sampler="fps"` in both calls; `point_indices` holds the rows taken.
    """

    def __init__(self, dataset, device):
        from wf3d import _lib
        from wf3d.ops import _stream
        self.ds, self.device = dataset, device
        self.ncol, (clo, chi) = _columns(dataset.use_color, dataset.use_intensity)
        raws = [_read_xyz(f)[:, :self.ncol] for f in dataset.pc_files]
        self.n = [r.shape[0] for r in raws]
        first = np.zeros(len(raws) + 1, dtype=np.int64)
        np.cumsum(self.n, out=first[1:])
        self.first = torch.from_numpy(first).to(device)
        raw = torch.from_numpy(np.ascontiguousarray(np.concatenate(raws, axis=0))).to(device)
        self.norm = torch.empty_like(raw)
        cen = torch.zeros(len(raws), 3, dtype=torch.float64, device=device)
        md = torch.ones(len(raws), dtype=torch.float64, device=device)
        lib = _lib.load()
        _lib.check(lib.wf3d_cloud_normalize(raw.data_ptr(), self.first.data_ptr(), len(raws), self.ncol, clo, chi,
                                            1 if dataset.normalize else 0, self.norm.data_ptr(), cen.data_ptr(), md.data_ptr(),
                                            _stream()), "cloud_normalize")
        self.centroid, self.max_distance = cen.cpu().numpy(), md.cpu().numpy()      # one read-back, at build time
        self.wireframes = [load_wireframe(f) for f in dataset.wireframe_files]
        # the wireframes resident too (wireframe_targets_kernel): vertices centred and scaled as batch() does per call
        verts = [self._normalised_vertices(i)[0] for i in range(len(raws))]
        edges = [np.asarray(e, dtype=np.int32).reshape(-1, 2) for _, e in self.wireframes]
        self.nv = [v.shape[0] for v in verts]
        vfirst, efirst = np.zeros(len(raws) + 1, dtype=np.int64), np.zeros(len(raws) + 1, dtype=np.int64)
        np.cumsum(self.nv, out=vfirst[1:])
        np.cumsum([e.shape[0] for e in edges], out=efirst[1:])
        self.wf_vertices = torch.from_numpy(np.ascontiguousarray(np.concatenate(verts, axis=0).reshape(-1, 3))).to(device)
        self.wf_edges = torch.from_numpy(np.ascontiguousarray(np.concatenate(edges, axis=0))).to(device)
        self.vfirst, self.efirst = torch.from_numpy(vfirst).to(device), torch.from_numpy(efirst).to(device)
        # the seed stream of the device sampler: a generator of the cache's own (never the dropout stream), keyed from
        # torch's CPU generator (two draws from it, here) and created now, so that it exists before any capture
        from wf3d.random import DropoutGenerator
        self.sample_generator = DropoutGenerator(device)
        self.last_sample_words = None

    def _normalised_vertices(self, idx):
        """(float64 copy of cloud idx's wireframe vertices, centred and scaled when the data set normalises; centroid; max_distance)"""
        wf_vertices = self.wireframes[idx][0].copy()
        cen = md = None
        if self.ds.normalize:
            cen, md = self.centroid[idx].copy(), self.max_distance[idx]
            wf_vertices -= cen
            wf_vertices /= md
        return wf_vertices, cen, md

    def _item(self, idx, fx, fy, rot, scale=None):
        """__getitem__'s dict for cloud idx under one augmentation draw (flips, rot = rotz(angle)), without its point cloud.
        scale: (sx, sy, sz) of the sample's extension row — the vertices follow the points."""
        ds = self.ds
        wf_vertices, cen, md = self._normalised_vertices(idx)
        if ds.augment:
            wf_vertices[:, 0] *= fx
            wf_vertices[:, 1] *= fy
            wf_vertices[:, 0:3] = np.dot(wf_vertices[:, 0:3], np.transpose(rot))
        if scale is not None:
            wf_vertices[:, 0:3] *= np.asarray(scale, dtype=np.float64)
        it = ds._finish(np.empty((0, self.ncol)), wf_vertices, self.wireframes[idx][1], cen, md, ds.pc_files[idx])
        del it["point_clouds"]
        return it

    def batch(self, indices, sampler="numpy", augment=None):
        """collate_batch([dataset[i] for i in indices]) with `point_clouds` [B, num_points, C] on the device.
        sampler="numpy": the rows are np.random.choice draws in the reference's order, so a seeded run reproduces the
        reference's batches.  sampler="device": the rows are chosen in the kernel (wf3d_cloud_sample_dev,
        wf3d.sampling.choice_indices) under a seed word drawn from `sample_generator` and kept as `last_sample_words`
        (int32 [5] on the device, word 0) — the same distribution, another random stream; np.random then sees the
        augmentation draws only (per sample flip-x, flip-y, angle), NO choice draws.  Every other key is the same.
        sampler="fps": as "device", with the rows by farthest-point sampling (wf3d_cloud_sample_fps,
        wf3d.sampling.fps_indices on the cloud's normalised xyz; the seed word picks the start row only), and one more
        key, `point_indices` (int32 [B, num_points] on the device): the rows taken.
        augment=cfg (sampler "device" or "fps" only): the extension of sampled_buffers for one batch — np.random sees, after
        the batch's draws above, per sample the scale value(s) and the dropout ratio (wf3d.sampling.ext_draws); the
        host-side wireframe fields are scaled like the points, and one more key, `aug_ext` (float64 [B, 8] on the device)."""
        from wf3d import _lib, sampling
        from wf3d.ops import _stream
        if sampler not in SAMPLERS:
            raise ValueError(f"DeviceCloudCache.batch: sampler must be 'numpy' or 'device', or 'fps' (got {sampler!r})")
        cfg = sampling.check_augment(augment)
        if cfg is not None and sampler == "numpy":
            raise ValueError("DeviceCloudCache.batch: augment= needs sampler='device' or 'fps' (jitter and dropout are keyed by "
                             "the device sampler's seed words, which sampler='numpy' does not have)")
        if not self.ds.num_points:
            raise ValueError("DeviceCloudCache needs dataset.num_points (fixed-size batches)")
        ds, P = self.ds, self.ds.num_points
        # the kernel indexes device arrays with these: normalise Python's negative indices and refuse anything out of
        # range here (the host arrays would wrap around silently, the device read would not)
        indices = [operator.index(i) for i in indices]
        indices = [i + len(self.n) if i < 0 else i for i in indices]
        if any(not 0 <= i < len(self.n) for i in indices):
            raise IndexError(f"DeviceCloudCache.batch: index out of range for {len(self.n)} clouds")
        B = len(indices)
        if sampler != "numpy":
            return self._batch_sampled(indices, P, sampler, cfg)
        choice = np.empty((B, P), dtype=np.int32)
        aug = np.empty((B, 4), dtype=np.float64)
        items = []
        for b, idx in enumerate(indices):
            n = self.n[idx]
            choice[b] = np.random.choice(n, P, replace=n < P)                     # same draws, same order as __getitem__
            fx, fy, angle = ds._draw_augmentation() if ds.augment else (1.0, 1.0, 0.0)
            aug[b] = (fx, fy, np.cos(angle), np.sin(angle))
            items.append(self._item(idx, fx, fy, rotz(angle)))
        out = ds.collate_batch(items)
        dev = self.device
        ids = torch.tensor(list(indices), dtype=torch.int32).to(dev, non_blocking=True)
        ch = torch.from_numpy(choice).to(dev, non_blocking=True)
        ag = torch.from_numpy(aug).to(dev, non_blocking=True)
        pcs = torch.empty(B, P, self.ncol, dtype=torch.float32, device=dev)
        _lib.check(_lib.load().wf3d_cloud_sample(self.norm.data_ptr(), self.first.data_ptr(), ids.data_ptr(), ch.data_ptr(),
                                                 ag.data_ptr(), B, P, self.ncol, pcs.data_ptr(), _stream()), "cloud_sample")
        out["point_clouds"] = pcs
        return out

    @staticmethod
    def _draw_ext(cfg, B):
        """float64 [B, 8]: the extension rows of a host-staged batch from np.random — per sample, in order, the scale
        value(s) (1, or 3 when anisotropic) and the dropout ratio, each drawn only where that part is configured
        (wf3d.sampling.ext_draws), the values one np.random.random() each would give, into wf3d.sampling.ext_rows"""
        from wf3d import sampling
        n_scale, n_drop = sampling.ext_draws(cfg)
        u = np.random.random((B, n_scale + n_drop))                # row-major: sample by sample, in the order above
        return sampling.ext_rows(cfg, u[:, :n_scale], u[:, n_scale] if n_drop else None)

    def _batch_sampled(self, indices, P, sampler, cfg=None):
        """batch(..., sampler="device" or "fps") behind its index checks"""
        ds, B = self.ds, len(indices)
        if not 1 <= B <= 4096 or B * P > 0x7FFFFFFF:
            raise ValueError(f"DeviceCloudCache.batch: sampler={sampler!r} needs 1 <= B <= 4096 and B * num_points < 2^31 (got {B} x {P})")
        block = torch.empty(PARAM_BYTES * B + 4, dtype=torch.uint8)
        v_aug, v_cloud, v_first = self._block_views(block, B)
        v_cloud[:], v_first[:] = indices, np.arange(B + 1, dtype=np.int64) * P
        draws = []
        for b, idx in enumerate(indices):
            fx, fy, angle = ds._draw_augmentation() if ds.augment else (1.0, 1.0, 0.0)
            v_aug[b] = (fx, fy, np.cos(angle), np.sin(angle))
            draws.append((fx, fy, angle))
        ext = self._draw_ext(cfg, B) if cfg is not None else None           # behind every draw the batch made before
        out = ds.collate_batch([self._item(idx, fx, fy, rotz(angle), None if ext is None else ext[b, :3])
                                for b, (idx, (fx, fy, angle)) in enumerate(zip(indices, draws))])
        pcs = torch.empty(B, P, self.ncol, dtype=torch.float32, device=self.device)
        self.last_sample_words = self.sample_generator.draw()
        fps = self._fps_tensors(B, P) if sampler == "fps" else {}
        ext_dev = torch.from_numpy(ext).to(self.device) if ext is not None else None
        self._sample(block.to(self.device), self.last_sample_words, pcs, fps, ext_dev)
        out["point_clouds"] = pcs
        if ext_dev is not None:
            out["aug_ext"] = ext_dev
        if fps:
            out["point_indices"] = fps["point_indices"]
        return out

    def _fps_tensors(self, B, P):
        """what farthest-point sampling writes beside the points: `point_indices` (int32 [B, P]: the rows taken), and
        `fps_workspace` when a resident cloud is longer than FPS_REG_ROWS (the library allocates nothing)"""
        from wf3d import _lib
        out = {"point_indices": torch.zeros(B, P, dtype=torch.int32, device=self.device)}
        nbytes = _lib.load().wf3d_cloud_sample_fps_ws_bytes(B, max(self.n))
        if nbytes:
            out["fps_workspace"] = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return out

    def _sample(self, params, words, points, fps=None, ext=None):
        """the sampler's launch: the random sampler, or farthest-point sampling into `fps`' tensors (_fps_tensors); with
        an extension block `ext` (float64 [B, 8] on the device) the `_ext` entry point of either"""
        from wf3d import _lib
        from wf3d.ops import _stream
        lib = _lib.load()
        B, P = points.shape[0], points.shape[1]
        more = () if ext is None else (ext.data_ptr(),)
        if fps:
            ws = fps.get("fps_workspace")
            _lib.check((lib.wf3d_cloud_sample_fps if ext is None else lib.wf3d_cloud_sample_fps_ext)(
                self.norm.data_ptr(), self.first.data_ptr(), len(self.n), params.data_ptr(), words.data_ptr(), B, P, self.ncol,
                points.data_ptr(), fps["point_indices"].data_ptr(), max(self.n), ws.data_ptr() if ws is not None else None,
                ws.numel() if ws is not None else 0, *more, _stream()), "cloud_sample_fps")
            return
        _lib.check((lib.wf3d_cloud_sample_dev if ext is None else lib.wf3d_cloud_sample_dev_ext)(
            self.norm.data_ptr(), self.first.data_ptr(), len(self.n), params.data_ptr(), words.data_ptr(), B, P, self.ncol,
            points.data_ptr(), *more, _stream()), "cloud_sample_dev")

    def _targets(self, buffers):
        """the targets' launch from the buffers' parameter block; the vertices follow the extension block's scale"""
        from wf3d import _lib
        from wf3d.ops import _stream
        lib = _lib.load()
        ext = buffers.get("aug_ext")
        B, V = buffers["vertices"].shape[0], buffers["vertices"].shape[1]
        _lib.check((lib.wf3d_wireframe_targets if ext is None else lib.wf3d_wireframe_targets_ext)(
            self.wf_vertices.data_ptr(), self.wf_edges.data_ptr(), self.vfirst.data_ptr(), self.efirst.data_ptr(), len(self.n),
            buffers["params"].data_ptr(), B, V, buffers["vertices"].data_ptr(), buffers["vertex_existence"].data_ptr(),
            buffers["vertex_counts"].data_ptr(), buffers["edge_labels"].data_ptr(), *(() if ext is None else (ext.data_ptr(),)),
            _stream()), "wireframe_targets")

    # ---- packed batches: whole clouds, one after the other ----------------------------------------------------------
    def _plan(self, indices, who, capacity=None, max_vertices=None, num_points=None):
        ds = self.ds
        return packed_plan(self.n, self.nv, indices, ds._draw_augmentation if ds.augment else None, capacity, max_vertices, who,
                           num_points)

    @staticmethod
    def _block_views(block, B):
        """(aug [B, 4] float64, cloud [B] int32, out_first [B + 1] int32) views of a host parameter block (include/wf3d.h)"""
        raw = block.numpy()
        return raw[:32 * B].view(np.float64).reshape(B, 4), raw[32 * B:36 * B].view(np.int32), raw[36 * B:].view(np.int32)

    def _pack(self, params, B, rows, points, point_counts):
        from wf3d import _lib
        from wf3d.ops import _stream
        _lib.check(_lib.load().wf3d_cloud_pack(self.norm.data_ptr(), self.first.data_ptr(), len(self.n), params.data_ptr(), B,
                                               rows, self.ncol, points.data_ptr(), point_counts.data_ptr(), _stream()), "cloud_pack")

    @staticmethod
    def _refuse_packed_augment(who, augment):
        from wf3d import sampling
        if sampling.check_augment(augment) is not None:
            raise ValueError(f"DeviceCloudCache.{who}: augment= is for fixed-size sampled batches only (sampled_buffers, "
                             "batch(sampler='device' | 'fps')): whole-cloud batches have no seed words under stage / fill")

    def packed_batch(self, indices, augment=None):
        """collate_packed([ds0[i] for i in indices]), ds0 = the data set with num_points = 0, with `point_clouds`
        [sum n_b, C] on the device; np.random is consumed as those __getitem__ calls consume it.  augment=: refused
        (ValueError), the extension is the sampled forms'."""
        self._refuse_packed_augment("packed_batch", augment)
        indices, out_first, aug = self._plan(indices, "packed_batch")
        B, rows = len(indices), int(out_first[-1])
        items = [self._item(idx, fx, fy, np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])) for idx, (fx, fy, c, s) in zip(indices, aug)]
        out = self.ds.collate_batch(items)
        block = torch.empty(PARAM_BYTES * B + 4, dtype=torch.uint8)
        v_aug, v_cloud, v_first = self._block_views(block, B)
        v_aug[:], v_cloud[:], v_first[:] = aug, indices, out_first
        points = torch.empty(rows, self.ncol, dtype=torch.float32, device=self.device)
        counts = torch.empty(B, dtype=torch.int64, device=self.device)
        self._pack(block.to(self.device), B, rows, points, counts)
        out["point_clouds"] = points
        out["point_counts"] = torch.tensor([self.n[i] for i in indices], dtype=torch.int64)
        return out

    def packed_buffers(self, B, capacity, max_vertices, augment=None):
        """Static device tensors of a captured step for batches of B whole clouds: `points` [capacity, C],
        `point_counts` int64 [B], train_targets' `vertices` / `vertex_existence` / `edge_labels` (full width) /
        `vertex_counts`, the parameter block `params` (uint8 [40 B + 4]) and its pinned host mirror `params_host`.
        augment=: refused (ValueError), the extension is the sampled forms'."""
        self._refuse_packed_augment("packed_buffers", augment)
        from wf3d.ops import check_capacity
        capacity = check_capacity(capacity)
        B, V = operator.index(B), operator.index(max_vertices)
        if not 1 <= B <= 4096 or V < 1:
            raise ValueError(f"DeviceCloudCache.packed_buffers: needs 1 <= B <= 4096 and max_vertices >= 1 (got {B}, {V})")
        dev = self.device
        f32 = dict(dtype=torch.float32, device=dev)
        return {"points": torch.zeros(capacity, self.ncol, **f32),
                "point_counts": torch.zeros(B, dtype=torch.int64, device=dev),
                "vertices": torch.zeros(B, V, 3, **f32),
                "vertex_existence": torch.zeros(B, V, **f32),
                "edge_labels": torch.zeros(B, V * (V - 1) // 2, **f32),
                "vertex_counts": torch.zeros(B, dtype=torch.int64, device=dev),
                "params": torch.zeros(PARAM_BYTES * B + 4, dtype=torch.uint8, device=dev),
                "params_host": torch.zeros(PARAM_BYTES * B + 4, dtype=torch.uint8).pin_memory(),
                "params_copied": torch.cuda.Event()}

    def sampled_buffers(self, B, max_vertices, num_points=None, sampler="device", augment=None):
        """Static device tensors of a captured step for FIXED-SIZE batches sampled on the device: `points`
        [B, P, C] (P = num_points or the data set's; the dense forward takes it as it is), train_targets' `vertices` /
        `vertex_existence` / `edge_labels` (full width) / `vertex_counts`, the parameter block `params` with its pinned
        mirror `params_host`, and `sample_words` (int32 [5]: the seed words `fill` draws, word 0 is the batch's).
        sampler="fps": the rows by farthest-point sampling (wf3d_cloud_sample_fps, wf3d.sampling.fps_indices) — the same
        buffers plus "sampler": "fps", `point_indices` (int32 [B, P]: the rows taken) and, when a resident cloud is
        longer than FPS_REG_ROWS, `fps_workspace`; stage / fill / fill_epoch dispatch on that key.
        augment=cfg (wf3d.sampling.check_augment; None or {}: nothing): a random scale, per-point jitter and random point
        dropout inside the sampler's launch, the vertices scaled with the points — three more entries, `augment` (the
        checked dict), `aug_ext` (float64 [B, 8] on the device: the extension block, identity rows at first) and
        `aug_ext_host` (its pinned mirror); stage / fill / fill_epoch dispatch on `aug_ext`.  Independent of the data
        set's `augment` (flips and rotation)."""
        from wf3d import sampling
        if sampler not in SAMPLERS[1:]:
            raise ValueError(f"DeviceCloudCache.sampled_buffers: sampler must be 'device' or 'fps' ('numpy' draws on the host: "
                             f"batch()) (got {sampler!r})")
        cfg = sampling.check_augment(augment)
        B, V = operator.index(B), operator.index(max_vertices)
        P = operator.index(num_points or self.ds.num_points or 0)
        if P < 1:
            raise ValueError("DeviceCloudCache.sampled_buffers: needs num_points or dataset.num_points")
        if not 1 <= B <= 4096 or V < 1 or B * P > 0x7FFFFFFF:
            raise ValueError(f"DeviceCloudCache.sampled_buffers: needs 1 <= B <= 4096, max_vertices >= 1 and B * num_points < 2^31 "
                             f"(got {B}, {V}, {P})")
        dev = self.device
        f32 = dict(dtype=torch.float32, device=dev)
        fps = dict(self._fps_tensors(B, P), sampler="fps") if sampler == "fps" else {}
        if cfg is not None:
            identity = torch.tensor(sampling.EXT_IDENTITY, dtype=torch.float64).repeat(B, 1)
            fps.update(augment=cfg, aug_ext=identity.to(dev), aug_ext_host=identity.clone().pin_memory())
        return {"points": torch.zeros(B, P, self.ncol, **f32),
                "vertices": torch.zeros(B, V, 3, **f32),
                "vertex_existence": torch.zeros(B, V, **f32),
                "edge_labels": torch.zeros(B, V * (V - 1) // 2, **f32),
                "vertex_counts": torch.zeros(B, dtype=torch.int64, device=dev),
                "params": torch.zeros(PARAM_BYTES * B + 4, dtype=torch.uint8, device=dev),
                "params_host": torch.zeros(PARAM_BYTES * B + 4, dtype=torch.uint8).pin_memory(),
                "params_copied": torch.cuda.Event(),
                "sample_words": torch.zeros(5, dtype=torch.int32, device=dev), **fps}

    def stage(self, buffers, indices):
        """Host only, outside any capture: check the batch against the buffers (IndexError / ValueError, nothing touched),
        draw its augmentation from np.random, fill the pinned mirror and issue ONE non-blocking copy of the parameter
        block.  Returns the batch's host-side fields `scan_idx`, `centroid`, `max_distance` as collate_batch builds them.
        `buffers` from packed_buffers or from sampled_buffers: the same checks (without the row capacity, which a
        fixed-size batch does not have) and the same draws in the same order — per sample flip-x, flip-y, angle.  The
        sampled form draws NO np.random.choice: it leaves np.random elsewhere than batch() does.
        Buffers with an extension (`aug_ext`): behind the batch's draws above, per sample and in order, the scale
        value(s) (1, or 3 when anisotropic; none when scale is (1, 1)) and the dropout ratio (none when max_dropout is 0),
        each one np.random.random() (wf3d.sampling.ext_row); the mirror `aug_ext_host` goes up by a second non-blocking
        copy in front of the same event.  Without one np.random is consumed exactly as before."""
        sampled = "sample_words" in buffers
        B = buffers["vertices"].shape[0]
        if len(indices) != B:
            raise ValueError(f"DeviceCloudCache.stage: {len(indices)} clouds for buffers of {B}")
        if sampled:
            indices, out_first, aug = self._plan(indices, "stage", None, buffers["vertices"].shape[1], buffers["points"].shape[1])
        else:
            indices, out_first, aug = self._plan(indices, "stage", buffers["points"].shape[0], buffers["vertices"].shape[1])
        buffers["params_copied"].synchronize()             # the mirror's last copy has left it (no wait when it has)
        v_aug, v_cloud, v_first = self._block_views(buffers["params_host"], B)
        v_aug[:], v_cloud[:], v_first[:] = aug, indices, out_first
        buffers["params"].copy_(buffers["params_host"], non_blocking=True)
        if "aug_ext" in buffers:
            buffers["aug_ext_host"].numpy()[:] = self._draw_ext(buffers["augment"], B)
            buffers["aug_ext"].copy_(buffers["aug_ext_host"], non_blocking=True)
        buffers["params_copied"].record()
        ds = self.ds
        info = {"scan_idx": torch.tensor(np.array([np.array(os.path.splitext(os.path.basename(ds.pc_files[i]))[0]).astype(np.int64)
                                                   for i in indices]))}
        if ds.normalize:
            info["centroid"] = torch.tensor(np.array([self.centroid[i] for i in indices]))
            info["max_distance"] = torch.tensor(np.array([self.max_distance[i] for i in indices]))
        return info

    def fill(self, buffers):
        """The two launches that fill `buffers` from the staged parameter block: every element of `points`, `point_counts`
        and the four target tensors is written.  Capturable: everything the kernels read is in device memory.
        Sampled buffers take three: a draw of `sample_generator` into `sample_words`, the sampler (every element of
        `points`), the targets — so every replay of a capture samples afresh.  Buffers with an extension (`aug_ext`): the
        same launches through the `_ext` entry points, which read the staged extension block."""
        B = buffers["vertices"].shape[0]
        if "sample_words" in buffers:
            self._sample(buffers["params"], self.sample_generator.draw(out=buffers["sample_words"]), buffers["points"],
                         buffers if buffers.get("sampler") == "fps" else None, buffers.get("aug_ext"))
        else:
            self._pack(buffers["params"], B, buffers["points"].shape[0], buffers["points"], buffers["point_counts"])
        self._targets(buffers)

    # ---- resident epochs: the batch order, the rank shards and the augmentation drawn on the device ---------------------
    def epoch_sampler(self, B, members=None, world=1, rank=0, seed=None):
        """An EpochSampler over `members` (resident cloud indices; all clouds by default, so one cache can hold several
        splits) for batches of B clouds per rank.  seed=None keys it from torch's CPU generator, at world == 1 only: the
        ranks of a data-parallel run must share one key, so world > 1 needs an explicit integer `seed`.  Create it
        before a capture starts."""
        return EpochSampler(self, B, members, world, rank, seed)

    def _check_epoch(self, buffers, sampler):
        """what stage() checks per batch, once for every batch the sampler can produce"""
        sampled = "sample_words" in buffers
        B, V = buffers["vertices"].shape[0], buffers["vertices"].shape[1]
        if sampler.cache is not self:
            raise ValueError("DeviceCloudCache.fill_epoch: the sampler belongs to another cache")
        if B != sampler.B:
            raise ValueError(f"DeviceCloudCache.fill_epoch: a sampler of {sampler.B} clouds per batch for buffers of {B}")
        members = sampler.members
        if members.min() < 0 or members.max() >= len(self.n):
            raise IndexError(f"DeviceCloudCache.fill_epoch: member out of range for {len(self.n)} clouds")
        most = max(self.nv[i] for i in set(members.tolist()))
        if most > V:
            raise ValueError(f"a wireframe has {most} vertices, more than max_vertices = {V}")
        if not sampled:
            rows = int(np.sort(np.asarray(self.n, dtype=np.int64)[members])[-B:].sum())
            if rows > buffers["points"].shape[0]:
                raise ValueError(f"DeviceCloudCache.fill_epoch: the {B} largest member clouds hold {rows} points, above the "
                                 f"capacity of {buffers['points'].shape[0]} rows")

    def fill_epoch(self, buffers, sampler):
        """fill() for the NEXT batch of `sampler`, with nothing made on the host: three launches — the parameter block
        and the seed words of batch t from the sampler's state (wf3d_cloud_epoch_params, which advances t), the sampler
        (`buffers` from sampled_buffers) or the pack kernel (from packed_buffers), the targets.  Capturable, and every
        replay advances to the next batch: no np.random draw, no pinned mirror, no copy.  The first call for a (buffers,
        sampler) pair checks, once and before any launch, what stage() checks per batch: every member is a resident cloud
        (IndexError), max_vertices holds the largest member wireframe and, for packed buffers, the capacity holds the B
        largest member clouds (ValueError) — so no batch can break the block's rules.
        Buffers with an extension (`aug_ext`): the same three launches through the `_ext` entry points — the first also
        writes the extension block from the buffers' `augment` (wf3d.sampling.epoch_augment_ext: scale and dropout ratio
        per (epoch, global slot), world-size invariant; jitter and the dropped rows per (step, rank))."""
        from wf3d import _lib, sampling
        from wf3d.ops import _stream
        sampled = "sample_words" in buffers
        B, V = buffers["vertices"].shape[0], buffers["vertices"].shape[1]
        pair = (buffers["params"].data_ptr(), buffers["points"].data_ptr(), tuple(buffers["points"].shape), V)
        if pair not in sampler._checked:
            self._check_epoch(buffers, sampler)
            sampler._checked.add(pair)
        lib = _lib.load()
        words = buffers["sample_words"] if sampled else sampler.seed_words
        ext = buffers.get("aug_ext")
        cfg8 = None if ext is None else sampling.augment_cfg8(buffers["augment"])      # host memory, read during the call
        _lib.check((lib.wf3d_cloud_epoch_params if ext is None else lib.wf3d_cloud_epoch_params_ext)(
            sampler.state.data_ptr(), sampler.members_dev.data_ptr(), len(sampler.members), self.first.data_ptr(), len(self.n), B,
            sampler.world, sampler.rank, buffers["points"].shape[1] if sampled else 0, 1 if self.ds.augment else 0,
            buffers["params"].data_ptr(), words.data_ptr(), *(() if ext is None else (cfg8.ctypes.data, ext.data_ptr())),
            _stream()), "cloud_epoch_params")
        if sampled:
            self._sample(buffers["params"], words, buffers["points"], buffers if buffers.get("sampler") == "fps" else None, ext)
        else:
            self._pack(buffers["params"], B, buffers["points"].shape[0], buffers["points"], buffers["point_counts"])
        self._targets(buffers)


def _as_int64(x):
    """the 64 bits of x as a signed integer (what an int64 tensor holds)"""
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >= 1 << 63 else x


class EpochSampler:
    """Shuffled, rank-sharded, augmented epochs over the member clouds of a DeviceCloudCache, from 16 bytes of device
    memory: `state` = int64 [key, t], t the batches produced so far.  `cache.fill_epoch(buffers, sampler)` reads it in the
    kernel and advances t, so a loop of graph.replay() calls with nothing between them walks the epochs;
    wf3d.sampling.epoch_batch states what batch t holds.

        sampler = cache.epoch_sampler(B, world=W, rank=r, seed=1234)       # before the capture
        with torch.cuda.graph(graph):
            cache.fill_epoch(buffers, sampler)                               # ... and the training step
        for _ in range(epochs * sampler.steps_per_epoch):
            graph.replay()

    steps_per_epoch = len(members) // (world * B): the last partial batch of an epoch is dropped.  The ranks' batches of
    a step are disjoint, and their union is the batch a single rank with batch world * B would get (same clouds, same
    augmentation).  The point rows a cloud contributes are keyed per (step, rank) and by the sample's position in the
    rank's batch: they are NOT invariant under the world size."""

    def __init__(self, cache, B, members=None, world=1, rank=0, seed=None):
        from wf3d import sampling
        B, world, rank = operator.index(B), operator.index(world), operator.index(rank)
        members = list(range(len(cache.n))) if members is None else [operator.index(i) for i in members]
        self.steps_per_epoch = sampling.epoch_steps(len(members), B, world, rank)
        if any(not -1 << 31 <= i < 1 << 31 for i in members):
            raise ValueError("DeviceCloudCache.epoch_sampler: a member is no int32")
        if seed is None:
            if world > 1:
                raise ValueError("DeviceCloudCache.epoch_sampler: world > 1 needs an explicit integer seed (the ranks share one key)")
        elif isinstance(seed, bool):
            raise ValueError("DeviceCloudCache.epoch_sampler: seed must be an integer or None")
        else:
            seed = operator.index(seed)
        if torch.device(cache.device).type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("DeviceCloudCache.epoch_sampler: the sampler must be created before a graph capture starts")
        if seed is None:                                                   # as wf3d.random.DropoutGenerator keys itself
            lo, hi = (int(x) for x in torch.randint(0, 1 << 32, (2,), dtype=torch.int64))
            seed = lo | (hi << 32)
        self.cache, self.B, self.world, self.rank = cache, B, world, rank
        self.key = seed & ((1 << 64) - 1)
        self.members = np.asarray(members, dtype=np.int32)
        self.members_dev = torch.from_numpy(self.members).to(cache.device)
        self.state = torch.tensor([_as_int64(self.key), 0], dtype=torch.int64, device=cache.device)
        self.seed_words = torch.zeros(5, dtype=torch.int32, device=cache.device)     # packed buffers have none of their own
        self._checked = set()

    def get_state(self):
        """[key, t] as a CPU int64 tensor (synchronises with the device)."""
        return self.state.detach().to("cpu", copy=True)

    def set_state(self, state):
        state = torch.as_tensor(state, dtype=torch.int64).cpu()
        if state.shape != (2,):
            raise ValueError(f"EpochSampler.set_state: an int64 tensor [key, t], got shape {tuple(state.shape)}")
        self.key = int(state[0]) & ((1 << 64) - 1)
        self.state.copy_(state)

    def seek(self, epoch, step=0):
        """The next batch is step `step` of epoch `epoch`."""
        epoch, step = operator.index(epoch), operator.index(step)
        if epoch < 0 or not 0 <= step < self.steps_per_epoch:
            raise ValueError(f"EpochSampler.seek: needs epoch >= 0 and 0 <= step < {self.steps_per_epoch} (got {epoch}, {step})")
        self.set_state(torch.tensor([_as_int64(self.key), _as_int64(epoch * self.steps_per_epoch + step)], dtype=torch.int64))

    def batch_at(self, t, augment_ext=None):
        """Batch number t as the specification gives it, on the host and without a sync: wf3d.sampling.epoch_batch's
        dict plus `cloud` (int32 [B]: the resident clouds).  A pure function of (key, t).  augment_ext=cfg (the
        `augment` of the buffers): also `ext` (float64 [B, 8]), the extension block fill_epoch writes."""
        from wf3d import sampling
        out = sampling.epoch_batch(self.key, t, len(self.members), self.B, self.world, self.rank, bool(self.cache.ds.augment),
                                   augment_ext)
        out["cloud"] = self.members[out["order"]]
        return out

    def block_at(self, t, num_points=0, augment_ext=None):
        """The parameter block of batch t (uint8 [40 B + 4], include/wf3d.h) as the kernel writes it: out_first = b *
        num_points for the fixed-size form, the clouds' row offsets for the packed form (num_points = 0).
        augment_ext=cfg: the pair (parameter block, extension block float64 [B, 8])."""
        spec, B, n = self.batch_at(t, augment_ext), self.B, self.cache.n
        block = torch.zeros(PARAM_BYTES * B + 4, dtype=torch.uint8)
        v_aug, v_cloud, v_first = DeviceCloudCache._block_views(block, B)
        v_aug[:], v_cloud[:] = spec["aug"], spec["cloud"]
        if num_points:
            v_first[:] = np.arange(B + 1, dtype=np.int64) * operator.index(num_points)
        else:
            rows = np.array([n[i] if 0 <= i < len(n) else 0 for i in spec["cloud"]], dtype=np.int64)
            v_first[0], v_first[1:] = 0, (np.cumsum(rows) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
        if "ext" in spec:
            return block, torch.from_numpy(spec["ext"].copy())
        return block
