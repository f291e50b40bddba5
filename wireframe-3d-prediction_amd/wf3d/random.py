"""Device-side dropout seeds: what makes a captured training step draw fresh masks on every replay.

With `wf3d.config.set_dropout_rng("device")` each train-mode edge-head forward in which some p > 0 launches one draw
kernel (csrc/random.hip) that reads this device's generator state — a 64-bit key and a 64-bit counter in device
memory — writes five seed words and advances the counter.  The mask kernels then load their seed from those words at
run time instead of taking it as a by-value kernel argument, so a graph captured around the step replays the draw
and every replay masks different elements.

    words[0] = s = low 32 bits of splitmix64(key, counter)        (formula in csrc/random.hip)
    words[k] = (s + k * 0x9E3779B9) mod 2^32, k = 1..4             the per-site seeds of EdgeFn.forward
                                                                   (oracle.dropout.site_seeds(words[0]) == words[1:])

The key comes from torch's CPU generator when a device's generator is created, so `torch.manual_seed` still makes a
run reproducible; `get_state()` / `set_state()` checkpoint the stream or clone it.  A generator must exist before a
capture starts (the warm-up steps create it): creating one inside a capture raises.
"""
import contextlib
import threading

import torch

from . import _lib
from ._lib import check
from .ops import _stream

_generators = {}
_tls = threading.local()


class DropoutGenerator:
    """The dropout seed stream of one device: state = int64 tensor [key, counter] on that device."""

    def __init__(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError(f"DropoutGenerator: a CUDA device, got {device}")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("wf3d.random: the device dropout generator must be created before a graph capture starts "
                               "(run a warm-up step first)")
        lo, hi = (int(x) for x in torch.randint(0, 1 << 32, (2,), dtype=torch.int64))
        key = lo | (hi << 32)
        key = key - (1 << 64) if key >= 1 << 63 else key                   # the same 64 bits as a signed int64
        self.device = device
        self.state = torch.tensor([key, 0], dtype=torch.int64, device=device)

    def draw(self, out=None):
        """Launch the draw kernel on the current stream: a fresh int32 [5] tensor of seed words, or `out` (a static
        int32 [5] tensor on this device: what a captured launch writes on every replay)."""
        if out is None:
            words = torch.empty(5, dtype=torch.int32, device=self.device)
        elif out.dtype != torch.int32 or out.shape != (5,) or out.device != self.device or not out.is_contiguous():
            raise ValueError(f"DropoutGenerator.draw: out must be a contiguous int32 [5] tensor on {self.device}")
        else:
            words = out
        check(_lib.load().wf3d_dropout_draw(self.state.data_ptr(), words.data_ptr(), _stream()), "dropout_draw")
        return words

    def get_state(self):
        """[key, counter] as a CPU int64 tensor (synchronises with the device)."""
        return self.state.detach().to("cpu", copy=True)

    def set_state(self, state):
        state = torch.as_tensor(state, dtype=torch.int64)
        if state.shape != (2,):
            raise ValueError(f"DropoutGenerator.set_state: an int64 tensor [key, counter], got shape {tuple(state.shape)}")
        self.state.copy_(state)


def default_generator(device):
    """The generator of `device`, created (and keyed from torch's CPU generator) on first use."""
    device = torch.device(device)
    idx = device.index if device.index is not None else torch.cuda.current_device()
    g = _generators.get(idx)
    if g is None:
        g = _generators[idx] = DropoutGenerator(torch.device("cuda", idx))
    return g


@contextlib.contextmanager
def seed_words(words):
    """Launches on this thread inside the block take their dropout seeds from `words` (int32 device tensor): every
    drop_seed argument is an index into it (wf3d_set_dropout_seed_words).  words = None: seeds by value."""
    prev = getattr(_tls, "words", None)
    ptr = words.data_ptr() if words is not None else None
    if ptr == prev:                                 # nothing to change (seeds by value: the default path)
        yield
        return
    lib = _lib.load()
    check(lib.wf3d_set_dropout_seed_words(ptr), "set_dropout_seed_words")
    _tls.words = ptr
    try:
        yield
    finally:
        check(lib.wf3d_set_dropout_seed_words(prev), "set_dropout_seed_words")
        _tls.words = prev
