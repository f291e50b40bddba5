"""Drop-in `datasets.building3d` (reference datasets/building3d.py:18-202) — row f-3, the input pipeline in
front of the hot path — plus its MI355X form, `DeviceCloudCache`.

`Building3DReconstructionDataset` keeps the reference's constructor, `__getitem__` dict (same keys, dtypes, values),
`collate_batch` and `load_files`, so `main.py` / `evaluate.py` / a torch DataLoader work unchanged; it draws from
`np.random` in the reference's order (sampling choice, then flip-x, flip-y, angle), so a seeded run reproduces the
reference's samples.  The .xyz text is read by the library's C parser instead of `np.loadtxt` (~30x faster).

`DeviceCloudCache(dataset, device)` is the resident form: every cloud is parsed once, uploaded as float64 (the raw
coordinates are UTM metres — fp32 cannot hold them), normalised once on the device (csrc/cloud.hip) and kept in HBM;
`cache.batch(indices)` then costs one small host->device copy of the random choices and ONE gather/augment kernel that
writes the model's `[B, num_points, C]` fp32 input directly — no per-sample file I/O, no per-sample host arrays."""
import ctypes
import glob
import operator
import os
from collections import defaultdict

import numpy as np
import torch
from torch.utils.data import Dataset


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


class DeviceCloudCache:
    """All clouds of a dataset resident in HBM, normalised once; batches are produced by one kernel.

        cache = DeviceCloudCache(dataset, torch.device("cuda:0"))
        batch = cache.batch([3, 0, 7])      # same dict as collate_batch([dataset[3], dataset[0], dataset[7]]), with
                                            # batch["point_clouds"] a device tensor; np.random is consumed identically
    """

    def __init__(self, dataset, device):
        from wf3d import _lib
        from wf3d.ops import _stream
        if not dataset.num_points:
            raise ValueError("DeviceCloudCache needs dataset.num_points (fixed-size batches)")
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

    def batch(self, indices):
        from wf3d import _lib
        from wf3d.ops import _stream
        ds, P = self.ds, self.ds.num_points
        # the kernel indexes device arrays with these: normalise Python's negative indices and refuse anything out of
        # range here (the host arrays would wrap around silently, the device read would not)
        indices = [operator.index(i) for i in indices]
        indices = [i + len(self.n) if i < 0 else i for i in indices]
        if any(not 0 <= i < len(self.n) for i in indices):
            raise IndexError(f"DeviceCloudCache.batch: index out of range for {len(self.n)} clouds")
        B = len(indices)
        choice = np.empty((B, P), dtype=np.int32)
        aug = np.empty((B, 4), dtype=np.float64)
        items = []
        for b, idx in enumerate(indices):
            n = self.n[idx]
            choice[b] = np.random.choice(n, P, replace=n < P)                     # same draws, same order as __getitem__
            fx, fy, angle = ds._draw_augmentation() if ds.augment else (1.0, 1.0, 0.0)
            aug[b] = (fx, fy, np.cos(angle), np.sin(angle))
            wf_vertices, wf_edges = self.wireframes[idx]
            wf_vertices = wf_vertices.copy()
            cen = md = None
            if ds.normalize:
                cen, md = self.centroid[idx].copy(), self.max_distance[idx]
                wf_vertices -= cen
                wf_vertices /= md
            if ds.augment:
                wf_vertices[:, 0] *= fx
                wf_vertices[:, 1] *= fy
                wf_vertices[:, 0:3] = np.dot(wf_vertices[:, 0:3], np.transpose(rotz(angle)))
            it = ds._finish(np.empty((0, self.ncol)), wf_vertices, wf_edges, cen, md, ds.pc_files[idx])
            del it["point_clouds"]
            items.append(it)
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
