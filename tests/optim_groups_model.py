"""A float64 model of the grouped step tail (wf3d_clip_adam_step_groups, wf3d.optim.ClipAdam with parameter groups),
built on tests/optim_model.py: ONE global norm and one clip coefficient over every tensor of every group and every
clip-only tensor, then per group its own lr, betas, eps, weight decay (L2, or decoupled as torch.optim.AdamW has it)
and its own Adam step.

  clip_adam_groups_step64(p, g, m, v, group, groups, max_norm)   one step -> (p', g', m', v', norm64), float64
  compare_groups_step(before, after, norm_kernel, ...)           optim_model.compare_step's bounds under this model

tests/test_optim_groups_model.py pins the model to torch in float64 and shows that the comparison rejects near misses;
tests/test_optim_groups_gpu.py holds the kernels to it."""
import numpy as np

import optim_model as OM

_single_step64 = OM.clip_adam_step64       # the single-group model every group's update goes through


def group_hp(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False, step=1):
    """One group's row: torch's hyper-parameters, the decay form, and the 1-based Adam step of its tensors."""
    return dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, decoupled=decoupled, step=step)


def clip_adam_groups_step64(p, g, m, v, group, groups, max_norm, norm=None):
    """One clip + Adam step over lists of arrays.  group[i]: tensor i's index into `groups` (rows of group_hp); None for
    a clip-only tensor (m[i] None: in the norm, gradient scaled, nothing else).  `norm`: evaluate the element-wise update
    under this global norm (the kernel's own) instead of the float64 one; norm64 is returned either way.

    Every group's update is optim_model.clip_adam_step64 over the group's tensors UNDER THE GLOBAL NORM.  A decoupled
    group runs it without weight decay (the gradient enters the moments as it is) and then takes lr * wd * p off the
    parameter it started from: p (1 - lr wd) - (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps), torch.optim.AdamW."""
    norm64 = OM.grad_norm64(g)
    used = norm64 if norm is None else float(norm)
    coef = OM.clip_coef64(used, max_norm)
    n = len(g)
    P, G, M, V = [None] * n, [None] * n, [None] * n, [None] * n
    with np.errstate(all="ignore"):
        for i in range(n):
            if m[i] is None:
                assert group[i] is None
                G[i] = np.asarray(g[i], dtype=np.float64) * coef
        for k, hp in enumerate(groups):
            idx = [i for i in range(n) if group[i] == k]
            if not idx:
                continue
            sub = [[x[i] for i in idx] for x in (p, g, m, v)]
            wd = 0.0 if hp["decoupled"] else hp["weight_decay"]
            Pk, Gk, Mk, Vk, _ = _single_step64(*sub, step=hp["step"], lr=hp["lr"], betas=hp["betas"], eps=hp["eps"],
                                              weight_decay=wd, max_norm=max_norm, norm=used)
            for j, i in enumerate(idx):
                P[i], G[i], M[i], V[i] = Pk[j], Gk[j], Mk[j], Vk[j]
                if hp["decoupled"] and hp["weight_decay"] != 0:
                    P[i] = P[i] - hp["lr"] * hp["weight_decay"] * np.asarray(p[i], dtype=np.float64)
    assert all(x is not None for x in G)
    return P, G, M, V, norm64


def compare_groups_step(before, after, norm_kernel, *, group, groups, max_norm):
    """optim_model.compare_step — its bounds on the norm, on g, m, v and on the UPDATE p' - p with the one rounding of
    the stored parameter, to the letter — with clip_adam_groups_step64 as the model it holds the step to.  compare_step
    reads its model through the module's name, so the grouped model stands in under that name for the one call."""
    def model(p, g, m, v, *, norm=None, **_):
        return clip_adam_groups_step64(p, g, m, v, group, groups, max_norm, norm=norm)

    OM.clip_adam_step64 = model
    try:
        return OM.compare_step(before, after, norm_kernel, step=0, lr=0.0, betas=(0.0, 0.0), eps=0.0, weight_decay=0.0,
                               max_norm=max_norm)
    finally:
        OM.clip_adam_step64 = _single_step64


# ---------------------------------------------------------------------------------------------------------------------
# the two groups and the inputs that the CPU sensitivity test and the GPU test share
# ---------------------------------------------------------------------------------------------------------------------
MAX_NORM = 1.0
# optim_model.HYPER's "defaults" and "moved" rows side by side: every hyper-parameter differs between the groups
TWO_GROUPS = (dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-6),
              dict(lr=1e-2, betas=(0.5, 0.9), eps=1e-3, weight_decay=0.1))
# optim_model.HYPER_SIZES = (1023, 16385, 5) interleaved: the group index is not monotonic in table order
TENSOR_GROUP = (0, 1, 0)
GROUP_STEPS = [(1, 1), (2, 2), (1000, 1000), (1000, 1)]        # the groups' Adam steps: together, and far apart
DECAY_FORMS = [(False, False), (False, True), (True, False)]   # which group decays decoupled


def two_groups(steps, decoupled=(False, False)):
    return [group_hp(step=s, decoupled=d, **hp) for hp, s, d in zip(TWO_GROUPS, steps, decoupled)]


def make_group_inputs(sizes, clip_only_sizes, tensor_group, steps, *, seed, norm, max_norm=MAX_NORM):
    """optim_model.make_inputs at the later of the groups' steps; the tensors of a group at step 1 get the zero moments
    that such a group has."""
    before = OM.make_inputs(sizes, clip_only_sizes, seed=seed, step=max(steps), norm=norm, max_norm=max_norm)
    for i, k in enumerate(tensor_group):
        if steps[k] == 1:
            before["m"][i] = np.zeros_like(before["m"][i])
            before["v"][i] = np.zeros_like(before["v"][i])
    return before
