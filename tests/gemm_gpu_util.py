"""What the element-by-element GEMM tests share on the device (tests/test_gemm_forms_gpu.py, tests/test_split_forms_gpu.py).

TEST INFRASTRUCTURE ONLY: poisoned buffers, operands placed inside them at a stride and a base offset, the workspace modes,
and the two assertions whose messages name the element, its tile, its K range and the kernel form (the caller's `where`).
"""
import contextlib

import numpy as np
import torch

POISON = 0x7FC0BEEF          # a quiet NaN with a payload: an untouched word is recognisable bit for bit
POISON_SX8 = 0x7FC07FC0      # the same for sx8 operands: both bf16 halves of the word are NaNs


def dev():
    return torch.device("cuda:0")


def poisoned(n, word=POISON):
    return torch.full((n,), word, dtype=torch.int32, device=dev()).view(torch.float32)


def place(arr, pad=0, off=0, word=POISON, tail=4):
    """A 2-D array as a device view with `pad` extra (poisoned) columns per row, `off` floats past an aligned base and
    `tail` poisoned floats behind the last row."""
    rows, cols = arr.shape
    ld = cols + pad
    buf = poisoned(off + rows * ld + tail, word)
    v = buf[off:off + rows * ld].view(rows, ld)[:, :cols]
    v.copy_(torch.from_numpy(arr))
    return v


def place1(arr, off=0):
    buf = poisoned(off + arr.shape[0] + 4)
    v = buf[off:off + arr.shape[0]]
    v.copy_(torch.from_numpy(arr))
    return v


@contextlib.contextmanager
def workspace(ops, mode, seen=None):
    """The workspace the wrappers in wf3d.ops hand to the library.  mode None: their own; "null": none at all; "short": one
    byte less than the library's query asks for; an int: that many bytes, whatever the query asks for.  seen: a list that
    receives (address, bytes) of every workspace handed out."""
    real = ops.scratch

    def scratch(nbytes, device, slot=0):
        if mode is None:
            ws = real(nbytes, device, slot)
        elif isinstance(mode, int):
            ws = real(mode, device, slot)[:mode]
        elif mode == "null" or nbytes <= 0:
            ws = None
        else:
            ws = real(nbytes, device, slot)[:nbytes - 1]
        if seen is not None:
            seen.append((ws.data_ptr(), ws.numel()) if ws is not None else (0, 0))
        return ws
    if mode is None and seen is None:
        yield
        return
    ops.scratch = scratch
    try:
        yield
    finally:
        ops.scratch = real


def assert_equal(name, tile, where, got, want, what):
    """torch.equal, or a message that names the first differing element through where(i, j) and the tiles touched."""
    if torch.equal(got, want):
        return
    bad = ~((got == want) | (got.isnan() & want.isnan()))
    idx = bad.nonzero()
    i, j = (int(v) for v in idx[0])
    tiles = sorted({(int(a) // tile[0], int(b) // tile[1]) for a, b in idx[:4096].tolist()})
    raise AssertionError(f"{name} [{what}]: {idx.shape[0]} of {got.numel()} elements differ; first at {where(i, j)}: "
                         f"got {float(got[i, j])!r}, want {float(want[i, j])!r}; tiles touched: {tiles[:12]}")


def assert_bound(name, where, got, ref, lim, S, what):
    """|got - ref| <= lim element by element (a non-finite error counts as infinite); prints the worst ratio."""
    g = got.double().cpu().numpy()
    err = np.abs(g - ref)
    err = np.where(np.isfinite(err), err, np.inf)
    ratio = err / np.maximum(lim, 1e-300)
    i, j = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    print(f"{name} [{what}]: worst |err| / bound = {ratio[i, j]:.3g}")
    assert ratio[i, j] <= 1.0, (f"{name} [{what}]: |got - ref| = {err[i, j]:.4g} > bound {lim[i, j]:.4g} (S = {S[i, j]:.4g}) at "
                                f"{where(i, j)}; {int((ratio > 1).sum())} elements over")
