"""Train-mode dropout of the three stages.  A stage takes it as an optional LAST argument after its parameters —
EncoderFn.apply(x, n_hidden, precision, *params, Drop(ps, seed)) — so that a call without one is the call it always was.
ps: the probability of every site of the stage in module order (encoder: mlp.{4i+3}; vertex head: vertex_mlp{k}.3; edge
head: vertex_proj.5, attention, edge_mlp.3, edge_mlp.7), each in [0, 1).  seed: the value the module drew on the host
(site k = 1, 2, ... masks with (seed + GOLDEN k) mod 2^32), or the five device seed words of wf3d.random (an int32
tensor; site k masks with words[k], so a draw serves WORD_SITES sites).  The mask of a site is wf3d_keep(site seed, row,
col): row = the row of the matrix the stage's Linears run on, col = the feature."""
import contextlib
from collections import namedtuple

import torch

from . import config
from .random import default_generator, seed_words

Drop = namedtuple("Drop", "ps seed")
GOLDEN = 0x9E3779B9
WORD_SITES = 4


def _take_drop(params, n_sites, who):
    """(params, ps, site seeds, device words or None) of a stage's trailing arguments.  No Drop, or one whose sites are all
    0: no site is active — ps all 0.0, no words, and every launch of the stage is the one without a mask."""
    drop = None
    if params and isinstance(params[-1], Drop):
        params, drop = params[:-1], params[-1]
    if drop is None or not any(drop.ps):
        return params, (0.0,) * n_sites, (0,) * n_sites, None
    ps = tuple(float(p) for p in drop.ps)
    if len(ps) != n_sites or not all(0.0 <= p < 1.0 for p in ps):
        raise ValueError(f"{who}: Drop.ps must be {n_sites} probabilities in [0, 1) (got {drop.ps})")
    if torch.is_tensor(drop.seed):
        if any(p > 0 for p in ps[WORD_SITES:]):
            raise ValueError(f"{who}: a draw of device seed words serves four dropout sites; site "
                             f"{max(k for k, p in enumerate(ps, 1) if p > 0)} is active (use the host seed mode, "
                             "wf3d.config.set_dropout_rng('host'))")
        return params, ps, tuple(range(1, n_sites + 1)), drop.seed
    return params, ps, tuple((int(drop.seed) + GOLDEN * k) & 0xFFFFFFFF for k in range(1, n_sites + 1)), None


def _seeded(words):
    """The seed source of a stage's launches: the device words of its Drop (set for this thread, forward and again in
    backward, which autograd runs on a thread of its own), or nothing to set."""
    return seed_words(words) if words is not None else contextlib.nullcontext()


def site_ps(owner, label, sites):
    """The probabilities of the dropout sites of `owner` (an nn.Module) in this call.  sites: its (site name, p) pairs in
    module order; label: what the messages call its stage.  All 0 outside train mode, whatever the modules hold."""
    if not owner.training:
        return (0.0,) * len(sites)
    ps = tuple([p for _, p in sites])
    if any(ps):                              # every site at 0: nothing to check
        for name, p in sites:
            if not 0.0 <= float(p) < 1.0:
                # torch would zero the whole site at p = 1; the dropout kernels take p in [0, 1)
                raise ValueError(f"{type(owner).__name__}: dropout p = {p} at {name} is not supported by the HIP {label} in "
                                 "train mode (needs 0 <= p < 1)")
    return ps


def module_drop(owner, label, sites, device):
    """The trailing arguments of this call's Function: nothing while no site is active (no seed is drawn, every launch is
    the one without a mask), else one Drop(ps, seed) — one draw per module and forward, from torch's CPU generator or,
    with dropout_rng "device", seed words drawn on the device (wf3d.random: no host read, fresh on every replay of a
    captured step).  The draw is recorded on the owner: last_dropout_seed / last_dropout_seeds."""
    ps = site_ps(owner, label, sites)
    if not any(ps):
        return ()
    if config.dropout_rng() == "device":
        late = [name for name, p in sites[WORD_SITES:] if p]
        if late:
            raise ValueError(f"{type(owner).__name__}: a draw of device seed words serves four dropout sites; {late[-1]} is "
                             "active (set it to 0, or use the host seed mode, wf3d.config.set_dropout_rng('host'))")
        seed = owner.last_dropout_seeds = default_generator(device).draw()
    else:
        seed = owner.last_dropout_seed = int(torch.empty((), dtype=torch.int64).random_().item())
    return (Drop(ps, seed),)
