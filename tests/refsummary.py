"""Compact, exact records of the reference's results for the fixtures under tests/golden/refcheck_*.npz.

A tensor the reference produced is stored whole up to FULL elements.  A larger one is stored as its max |a|, a fixed
seeded sample of SAMPLE elements, and the sums of its rows and of its columns (of the 2-D view `view2d`), taken over at
most BLOCKS runs of consecutive rows / columns.  Every check `violations` makes follows from the element-wise bound it
stands for, max |a - b| <= rtol * max |b| + atol:
  - sampled (or all) elements:  |a_i - b_i|            <= rtol * s + atol
  - the tensor's max |.|:       | max|a| - max|b| |     <= rtol * s + atol
  - a block sum of n elements:  |sum (a_i - b_i)|      <= n * (rtol * s + atol)
with s = max |b| of the reference.  Parameters and regenerated inputs are pinned bit for bit by `digest`.

This module has no side effects on sys.path: the fixture generators import it next to the reference's packages."""
import hashlib
import zlib

import numpy as np
import torch

FULL = 1024
SAMPLE = 512
BLOCKS = 128


def as_np(a):
    if torch.is_tensor(a):
        a = a.detach().cpu().numpy()
    return np.asarray(a)


def digest(a):
    """shape, dtype and sha256 of the bytes: bit-exact identity of a tensor."""
    a = np.ascontiguousarray(as_np(a))
    return f"{a.shape}|{a.dtype}|{hashlib.sha256(a.tobytes()).hexdigest()}"


def view2d(a):
    a = np.asarray(a, dtype=np.float64)
    if a.ndim >= 2:
        return a.reshape(a.shape[0], -1)
    a = a.reshape(-1)
    return np.pad(a, (0, (-a.size) % 64)).reshape(-1, 64)


def block_sums(v, axis):
    """Sums of `v` over blocks of consecutive rows (axis 0) / columns (axis 1), and the element count of each block."""
    m = v.shape[axis]
    starts = np.unique(np.linspace(0, m, min(m, BLOCKS), endpoint=False).astype(np.int64))
    sums = np.add.reduceat(v.sum(1 - axis), starts)
    return sums, np.diff(np.append(starts, m)) * v.shape[1 - axis]


def sample_index(name, n):
    rng = np.random.default_rng([7, zlib.crc32(name.encode())])
    return np.sort(rng.choice(n, SAMPLE, replace=False))


def summarize(name, a, out):
    """Write the record of array `a` under `name.*` into the dict `out`."""
    a = as_np(a)
    out[name + ".shape"] = np.array(a.shape, dtype=np.int64)
    out[name + ".maxabs"] = np.array(float(np.abs(a).max()) if a.size else 0.0)
    if a.size <= FULL:
        out[name + ".full"] = a.copy()
        return
    out[name + ".sample"] = a.reshape(-1)[sample_index(name, a.size)].copy()
    v = view2d(a)
    out[name + ".rows"] = block_sums(v, 0)[0].astype(np.float32)
    out[name + ".cols"] = block_sums(v, 1)[0].astype(np.float32)


def violations(gold, name, a, rtol, atol=0.0, floor=0.0):
    """[] if `a` is consistent with the record `name` under max|a - ref| <= rtol * max(s, floor) + atol; else what fails."""
    a = as_np(a)
    shape = tuple(int(d) for d in gold[name + ".shape"])
    if a.shape != shape:
        return [(name, "shape", a.shape, shape)]
    s = float(gold[name + ".maxabs"])
    tol = rtol * max(s, floor) + atol
    a64 = a.astype(np.float64)
    bad = []
    if name + ".full" in gold:
        d = float(np.abs(a64 - gold[name + ".full"]).max()) if a.size else 0.0
        if d > tol:
            bad.append((name, "element", d, tol))
        return bad
    d = float(np.abs(a64.reshape(-1)[sample_index(name, a.size)] - gold[name + ".sample"]).max())
    if d > tol:
        bad.append((name, "sampled element", d, tol))
    d = abs(float(np.abs(a64).max()) - s)
    if d > tol:
        bad.append((name, "max |.|", d, tol))
    v = view2d(a64)
    for part, axis in (("rows", 0), ("cols", 1)):
        got, n = block_sums(v, axis)
        # the stored sums are float32: their own rounding (2^-24 of |sum| <= n s) is added to the bound
        d = np.abs(got - gold[name + "." + part].astype(np.float64)) - n * s * 2.0 ** -24
        if float((d / n).max()) > tol:
            bad.append((name, part + " sums", float((d / n).max()), tol))
    return bad
