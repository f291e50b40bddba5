"""Synthetic, seeded inputs of the resident data set kernel tests (tests/test_cloud_kernels_gpu.py, tests/test_cloud_model.py):
building-like clouds and resident wireframes with every kind of edge list."""
import itertools

import numpy as np

OFFSET = np.array([532215.38, 6589285.65, 7.67])        # a building of the data set: UTM metres
ROWS = (1, 2, 3, 255, 256, 257, 513, 1300)              # idle lanes, one full pass, a tail iteration, several passes
COLOR_RANGE = {3: (0, 0), 7: (3, 7), 8: (3, 7), 4: (0, 0), 16: (0, 0)}          # the project's column modes; 4 and 16: none


def building_cloud(rng, n, C):
    """[n, C] float64: xyz within +-12 m of OFFSET rounded to 4 decimals (as the .xyz files hold them), colours 0..255,
    intensity up to 6e4, further columns uniform"""
    cols = [np.round(OFFSET + rng.uniform(-12.0, 12.0, (n, 3)), 4)]
    if C > 3:
        cols.append(rng.randint(0, 256, (n, min(C, 7) - 3)).astype(np.float64))
    if C > 7:
        cols.append(rng.uniform(0.0, 6e4, (n, 1)))
    if C > 8:
        cols.append(rng.uniform(-1.0, 1.0, (n, C - 8)))
    return np.ascontiguousarray(np.concatenate(cols, axis=1))


def plant_farthest(cloud, row):
    """move `row` well outside the +-12 m box: the cloud's farthest point from any centroid inside the box"""
    cloud[row, :3] = np.round(OFFSET + np.array([40.0, -35.0, 30.0]), 4)
    return cloud


def packed(clouds):
    """(table [sum n, C], first [nclouds + 1] int64) of a list of [n, C] clouds; a cloud of no rows is np.empty((0, C))"""
    first = np.zeros(len(clouds) + 1, dtype=np.int64)
    np.cumsum([c.shape[0] for c in clouds], out=first[1:])
    return np.ascontiguousarray(np.concatenate(clouds, axis=0)), first


def normalize_clouds(C, seed=3):
    """the clouds of one normalise launch: ROWS with a cloud of no rows between two of them, then 513-row clouds with the
    farthest point planted at row 0, n - 1, 255 and 256.  Returns (list of clouds, {name: cloud index})"""
    rng = np.random.RandomState(seed + C)
    clouds, names = [], {}
    for n in ROWS:
        if n == 255:
            names["empty"] = len(clouds)
            clouds.append(np.empty((0, C)))
        names[n] = len(clouds)
        clouds.append(building_cloud(rng, n, C))
    for row in (0, 512, 255, 256):
        names[f"far{row}"] = len(clouds)
        clouds.append(plant_farthest(building_cloud(rng, 513, C), row))
    return clouds, names


def all_pairs(c):
    return list(itertools.combinations(range(c), 2))


def wireframes(seed=5):
    """Resident wireframes (vertices [c, 3] float64 in the normalised unit ball, edges [e, 2] int32) with c in
    {0, 1, 2, 3, 16, 17, 300} and edge lists: none, all pairs, every pair reversed, duplicates, self loops, a negative
    index, the indices c and c + 5, and 600 edges for c = 300.  Returns (list of (vertices, edges), {name: index})."""
    rng = np.random.RandomState(seed)

    def verts(c):
        return rng.uniform(-1.0, 1.0, (c, 3))

    def junk(c):                                     # edges no candidate list holds
        return [(0, 0), (c - 1, c - 1), (-1, 0), (0, -1), (0, c), (c, 0), (1, c + 5), (c, c + 5)]

    sets = {
        "c0": (0, [(0, 5), (0, 0)]),                                   # no vertex: every edge is out of range
        "c1": (1, junk(1)),
        "c2_reversed_twice": (2, [(1, 0), (1, 0), (0, 1)]),
        "c3_none": (3, []),
        "c3_all_reversed": (3, [(j, i) for i, j in all_pairs(3)]),
        "c16_all": (16, all_pairs(16)),
        "c16_mixed": (16, junk(16) + all_pairs(16)[::3] + [(j, i) for i, j in all_pairs(16)[::5]] + all_pairs(16)[::3]),
        "c17": (17, junk(17) + [(16, 3), (2, 16), (15, 16)] + all_pairs(17)[::4]),
        "c300": (300, None),
    }
    out, names = [], {}
    for name, (c, edges) in sets.items():
        if edges is None:                            # 600 edges: random pairs (both orders, some repeated), some invalid
            e = rng.randint(0, c, (600, 2))
            e[:40] = e[40:80][:, ::-1]
            e[80:90] = [[-1, 5]] * 5 + [[c, 2]] * 3 + [[7, c + 5]] * 2
            e[-1] = (c - 2, c - 1)                   # the last pair of all
            e[-2] = (0, 1)
            edges = e
        names[name] = len(out)
        out.append((verts(c), np.asarray(edges, dtype=np.int32).reshape(-1, 2)))
    return out, names


def resident_wireframes(wfs):
    """(wf_vertices [sum c, 3], wf_edges [sum e, 2] int32, vfirst, efirst) of a list of (vertices, edges)"""
    v, vfirst = packed([w[0].reshape(-1, 3) for w in wfs])
    e, efirst = packed([w[1].reshape(-1, 2) for w in wfs])
    return v, np.ascontiguousarray(e.astype(np.int32)), vfirst, efirst


AUGS = {"identity": lambda rng, B: np.tile([1.0, 1.0, 1.0, 0.0], (B, 1)),
        "flips": lambda rng, B: np.array([[(1.0, -1.0)[b & 1], (-1.0, 1.0, 1.0, -1.0)[b & 3], 1.0, 0.0] for b in range(B)]).reshape(B, 4),
        "rotation": lambda rng, B: _rotations(rng, B)}


def _rotations(rng, B):
    """the data set's draws: flips at random, an angle within +-5 degrees"""
    t = rng.uniform(-np.pi / 36, np.pi / 36, B)
    return np.stack([rng.choice([-1.0, 1.0], B), rng.choice([-1.0, 1.0], B), np.cos(t), np.sin(t)], axis=1)


def augmentation(kind, B, seed=0):
    return np.ascontiguousarray(AUGS[kind](np.random.RandomState(100 + seed), B), dtype=np.float64)
