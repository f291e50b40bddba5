"""The index function of the device sampler (csrc/cloud.hip, cloud_sample_dev kernels), stated once in numpy: the
specification the kernel is tested against.  No GPU, no torch.

`choice_indices(seed_word, b, n, P)` is what `np.random.choice(n, P, replace=n < P)` is to the host pipeline — P row
indices of a cloud of n rows, distinct when n >= P — but computable per output position with O(1) state, no scratch
and no sort, so a kernel produces a fixed-size batch in one gather pass.  It is ANOTHER random stream than numpy's: the
same distribution of subsets, not the same subsets.

    fmix32(x)    murmur3's 32-bit finaliser: x ^= x >> 16; x *= 0x85EBCA6B; x ^= x >> 13; x *= 0xC2B2AE35; x ^= x >> 16
    mulhi(x, n)  floor(x * n / 2^32): a 32-bit word scaled to [0, n)
    key  = fmix32(fmix32(seed_word + 0x9E3779B9) ^ ((b + 1) * 0x85EBCA6B))        one per sample of a batch
    key2 = fmix32(key ^ 0x68E31DA4)
    a    = mulhi(fmix32(key ^ 0xB5297A4D), n),  c = mulhi(fmix32(key ^ 0x1B56C4E9), n)

  n >= P, without replacement:   idx[p] = (pi((p + a) mod n) + c) mod n
    pi = a keyed balanced Feistel permutation of 2h bits, h = ceil(bitlen(n - 1) / 2) (its domain 4^h lies in [n, 4n)),
    cycle-walked into [0, n): applied again while the value is >= n.  A permutation of [0, 4^h) restricted this way is
    a permutation of [0, n), and the walk ends after at most 4^h - n + 1 applications (fewer than 4 expected).
    Six rounds, (L, R) <- (R, L ^ (fmix32(R * 0x9E3779B1 + key + round * 0x7F4A7C15) & (2^h - 1))), L the high half.
    The offsets a and c make every position's marginal uniform whatever pi is (idx[p] is a fixed value plus c mod n);
    the joint statistics are the Feistel network's.
  n < P, with replacement:       idx[p] = mulhi(fmix32(fmix32(p ^ key) + key2), n)

All arithmetic is modulo 2^32 (the kernel's uint32); the only wide product is the multiply-high.  Limits: 1 <= n < 2^31,
1 <= P.  "Uniform" is up to the 2^-32 granularity of the multiply-high (a relative bias below n / 2^32).

Below it, the specification of the epoch sampler (cloud_epoch_params_kernel): `epoch_batch(key, t, D, B, world, rank)`,
and of farthest-point sampling (cloud_fps_kernel): `fps_indices(seed_word, b, xyz, P)`, the rows by distance.  At the
end, the augmentation extension of the sampled forms (the `_ext` entry points): scale, jitter and point dropout.
"""
import numpy as np

ROUNDS = 6
_M = np.uint64(0xFFFFFFFF)


def _u(x):
    return np.uint64(x)


def fmix32(x):
    x = np.asarray(x, dtype=np.uint64) & _M
    x = x ^ (x >> _u(16))
    x = (x * _u(0x85EBCA6B)) & _M
    x = x ^ (x >> _u(13))
    x = (x * _u(0xC2B2AE35)) & _M
    return x ^ (x >> _u(16))


def mulhi(x, n):
    return (np.asarray(x, dtype=np.uint64) * _u(n)) >> _u(32)


def half_bits(n):
    """h: the Feistel network works on 2h bits, the even width that holds n - 1."""
    return (int(n - 1).bit_length() + 1) // 2


def sample_keys(seed_words, b):
    """(key, key2) of sample b under each seed word."""
    s = np.asarray(seed_words, dtype=np.uint64) & _M
    key = fmix32(fmix32((s + _u(0x9E3779B9)) & _M) ^ _u(((int(b) + 1) * 0x85EBCA6B) & 0xFFFFFFFF))
    return key, fmix32(key ^ _u(0x68E31DA4))


def feistel(x, key, h):
    """One application of pi on [0, 4^h); x and key broadcast."""
    mask = _u((1 << h) - 1)
    left, right = x >> _u(h), x & mask
    for r in range(ROUNDS):
        f = fmix32((right * _u(0x9E3779B1) + key + _u((r * 0x7F4A7C15) & 0xFFFFFFFF)) & _M) & mask
        left, right = right, left ^ f
    return (left << _u(h)) | right


def choice_indices_many(seed_words, b, n, P, return_walks=False):
    """choice_indices for every seed word of a sequence at once: int64 [S, P].  return_walks: also the longest cycle
    walk (applications of pi for one index) and the applications in all, (0, 0) with replacement."""
    n, P = int(n), int(P)
    if not (1 <= n < 1 << 31 and P >= 1):
        raise ValueError(f"choice_indices: needs 1 <= n < 2^31 and P >= 1 (got n = {n}, P = {P})")
    key, key2 = sample_keys(np.atleast_1d(seed_words), b)
    key, key2 = key[:, None], key2[:, None]
    p = np.arange(P, dtype=np.uint64)[None, :]
    if n < P:
        idx = mulhi(fmix32((fmix32(p ^ key) + key2) & _M), n)
        return (idx.astype(np.int64), 0, 0) if return_walks else idx.astype(np.int64)
    a, c = mulhi(fmix32(key ^ _u(0xB5297A4D)), n), mulhi(fmix32(key ^ _u(0x1B56C4E9)), n)
    h, nn = half_bits(n), _u(n)
    x = feistel((p + a) % nn, key, h)
    flat, keys, walks, total = x.reshape(-1), np.broadcast_to(key, x.shape).reshape(-1), 1, x.size
    out = np.flatnonzero(flat >= nn)                     # the positions still outside [0, n): walk them on
    while out.size:
        step = feistel(flat[out], keys[out], h)
        flat[out] = step
        out = out[step >= nn]
        walks += 1
        total += step.size
    idx = ((x + c) % nn).astype(np.int64)
    return (idx, walks, total) if return_walks else idx


def choice_indices(seed_word, b, n, P):
    """int64 [P]: the rows sample `b` of a batch takes from a cloud of n rows under the batch's 32-bit `seed_word`."""
    return choice_indices_many([int(seed_word) & 0xFFFFFFFF], b, n, P)[0]


# ---------------------------------------------------------------------------------------------------------------------
# Resident epochs (csrc/cloud.hip, cloud_epoch_params_kernel): which clouds a batch holds, their augmentation and the row
# sampler's seed words as a pure function of a 64-bit key and the batch number t.
#
#   mix64(key, n)   csrc/random.hip's splitmix64 step: z = key + (n + 1) * 0x9E3779B97F4A7C15;
#                   z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31  (mod 2^64)
#   D member clouds, B per rank, W ranks, rank r:  S = D // (W B) steps per epoch (the last partial batch is dropped)
#   batch t:  e = t // S, s = t % S;  slot b's global slot g = s W B + r B + b
#   order_e  = choice_indices(low32(mix64(key, e)), 0, D, D)          a permutation of [0, D) per epoch
#   cloud[b] = members[order_e[g]]
#   c = e 2^32 + g:  za = mix64(key ^ 0x6A09E667F3BCC908, c): flip_x = -1 iff bit 63, flip_y = -1 iff bit 62
#                    u = (mix64(key ^ 0xBB67AE8584CAA73B, c) >> 11) 2^-53;  t_rot = u (pi / 18) - pi / 36
#   cos, sin of t_rot: epoch_cos_sin, fixed polynomials with every operation rounded on its own
#   seed words: s = low32(mix64(key ^ 0x3C6EF372FE94F82B, t W + r)), words[k] = s + k 0x9E3779B9 (k = 0..4)
#
# Slots and augmentation depend on (e, g) only: the W ranks' batches of a step are disjoint and their union is the batch
# of ONE rank with batch W B.  The seed words are per (step, rank), and the row sampler keys sample b by its LOCAL b, so
# the ROWS a cloud contributes are not world-size invariant.  Limits: 1 <= D < 2^31, 1 <= B <= 4096, 0 <= r < W, W B <= D.
# ---------------------------------------------------------------------------------------------------------------------
_M64 = (1 << 64) - 1
KEY_FLIP, KEY_ANGLE, KEY_ROWS = 0x6A09E667F3BCC908, 0xBB67AE8584CAA73B, 0x3C6EF372FE94F82B
MAX_EPOCH_BATCH = 4096


def mix64(key, n):
    """uint64 array: the splitmix64 step at position(s) n of key's stream; key and n broadcast (any integers, mod 2^64)."""
    def words(v):
        if isinstance(v, np.ndarray) and v.dtype.kind in "iu":          # two's complement: the same as & (2^64 - 1)
            return np.atleast_1d(v).astype(np.uint64)
        return np.asarray([int(k) & _M64 for k in np.atleast_1d(v).tolist()], dtype=np.uint64)
    key, n = words(key), words(n)
    with np.errstate(over="ignore"):
        z = key + (n + _u(1)) * _u(0x9E3779B97F4A7C15)
        z = (z ^ (z >> _u(30))) * _u(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _u(27))) * _u(0x94D049BB133111EB)
    return z ^ (z >> _u(31))


def epoch_steps(D, B, world=1, rank=0):
    """S = D // (world * B), the steps of an epoch, behind the limits (ValueError)."""
    D, B, world, rank = int(D), int(B), int(world), int(rank)
    if not 1 <= D < 1 << 31:
        raise ValueError(f"epoch sampler: needs 1 <= D < 2^31 member clouds (got {D})")
    if not 1 <= B <= MAX_EPOCH_BATCH:
        raise ValueError(f"epoch sampler: needs 1 <= B <= {MAX_EPOCH_BATCH} (got {B})")
    if world < 1 or not 0 <= rank < world:
        raise ValueError(f"epoch sampler: needs 0 <= rank < world (got rank {rank}, world {world})")
    if world * B > D:
        raise ValueError(f"epoch sampler: world * B = {world * B} passes the {D} member clouds: no whole step in an epoch")
    return D // (world * B)


def epoch_order(key, e, D):
    """int64 [D]: the order in which epoch e visits the members, a permutation of [0, D)."""
    return choice_indices(int(mix64(key, e)[0]) & 0xFFFFFFFF, 0, D, D)


def epoch_cos_sin(t):
    """(cos t, sin t) for |t| <= pi / 36 as fixed polynomials — Taylor's, by Horner's rule, to x^12 and x^13 — with every
    operation rounded on its own, so that the kernel (no fma) gives the same bits.  Truncation < 1e-25 on that range."""
    t = np.asarray(t, dtype=np.float64)
    x = t * t
    ps, pc = np.ones_like(t), np.ones_like(t)
    for k in (13, 11, 9, 7, 5, 3):
        ps = 1.0 - x * ps / float(k * (k - 1))
    for k in (12, 10, 8, 6, 4, 2):
        pc = 1.0 - x * pc / float(k * (k - 1))
    return pc, t * ps


def epoch_augmentation(key, e, g, augment=True):
    """float64 [len(g), 4] {flip_x, flip_y, cos t_rot, sin t_rot} of the global slots g of epoch e, and t_rot [len(g)]."""
    g = np.atleast_1d(np.asarray(g, dtype=np.int64))
    aug = np.tile(np.array([1.0, 1.0, 1.0, 0.0]), (g.size, 1))
    if not augment:
        return aug, np.zeros(g.size)
    c = [((int(e) << 32) + int(k)) & _M64 for k in g]
    za, zb = mix64(int(key) ^ KEY_FLIP, c), mix64(int(key) ^ KEY_ANGLE, c)
    aug[:, 0] = np.where((za >> _u(63)) & _u(1), -1.0, 1.0)
    aug[:, 1] = np.where((za >> _u(62)) & _u(1), -1.0, 1.0)
    u = (zb >> _u(11)).astype(np.float64) * 2.0 ** -53
    t_rot = u * (np.pi / 18) - np.pi / 36
    aug[:, 2], aug[:, 3] = epoch_cos_sin(t_rot)
    return aug, t_rot


def epoch_seed_words(key, t, world=1, rank=0):
    """uint32 [5]: the seed words of batch t on `rank` (word 0 is the row sampler's)."""
    s = int(mix64(int(key) ^ KEY_ROWS, int(t) * int(world) + int(rank))[0]) & 0xFFFFFFFF
    return np.array([(s + k * 0x9E3779B9) & 0xFFFFFFFF for k in range(5)], dtype=np.uint32)


def epoch_batch(key, t, D, B, world=1, rank=0, augment=True, augment_ext=None):
    """Batch number t >= 0 of the sampler keyed `key`: a dict of `epoch`, `step`, `slots` (int64 [B]: the global slots g),
    `order` (int64 [B]: order_e[g], positions in the member table), `aug` (float64 [B, 4]), `angle` (float64 [B]: t_rot)
    and `seed_words` (uint32 [5]); with a configuration `augment_ext` (check_augment) also `ext` (float64 [B, 8]:
    epoch_augment_ext of the slots)."""
    S = epoch_steps(D, B, world, rank)
    key, t = int(key) & _M64, int(t)
    if not 0 <= t <= _M64:
        raise ValueError(f"epoch sampler: the batch number is a uint64 (got {t})")
    e, s = divmod(t, S)
    g = s * world * B + rank * B + np.arange(B, dtype=np.int64)
    aug, angle = epoch_augmentation(key, e, g, augment)
    out = {"epoch": e, "step": s, "slots": g, "order": epoch_order(key, e, D)[g], "aug": aug, "angle": angle,
           "seed_words": epoch_seed_words(key, t, world, rank)}
    if check_augment(augment_ext) is not None:
        out["ext"] = epoch_augment_ext(key, e, g, augment_ext)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# Farthest-point sampling (csrc/cloud.hip, cloud_fps kernels): the rows of a fixed-size batch chosen by distance instead
# of by chance.  One start point per (seed word, sample), then P - 1 dependent rounds of "lower every point's distance to
# the picked set, take the farthest".  Specified bit for bit: float64, every operation rounded on its own (no fma), in
# ONE association, and the lowest index among equal distances — so lattices and coincident points are determined too.
# ---------------------------------------------------------------------------------------------------------------------
def fps_start(seed_word, b, n):
    """The first row sample `b` takes from a cloud of n rows under `seed_word`: mulhi(fmix32(key ^ 0xB5297A4D), n), the
    offset `a` of choice_indices — uniform on [0, n)."""
    n = int(n)
    if not 1 <= n < 1 << 31:
        raise ValueError(f"fps_start: needs 1 <= n < 2^31 (got n = {n})")
    key = sample_keys([int(seed_word) & 0xFFFFFFFF], b)[0]
    return int(mulhi(fmix32(key ^ _u(0xB5297A4D)), n)[0])


def fps_order(xyz, start, L):
    """int64 [L]: the first L rows of the farthest-point order of xyz (float64 [n, 3], 1 <= L <= n) from row `start`.

    order[0] = start.  Every point carries d, +inf at first.  After picking s: d[s] = -1 (a picked point is never picked
    again), and for every other i, r = ((x_i - x_s)^2 + (y_i - y_s)^2) + (z_i - z_s)^2 — each subtraction, product and
    sum rounded to float64 on its own, in this association — and d[i] = r if r < d[i].  The next pick is the index of
    the largest d, the LOWEST index among equals.  fps_order(xyz, start, n) is a permutation of [0, n), and a shorter
    order is its prefix.

    Non-finite coordinates: a NaN r never lowers a d (the comparison is false), so a point with a NaN or two infinities
    of a kind keeps d = +inf until it is picked, which is early; while it is the picked point no d moves.  Every index
    stays in range and the loop ends after L rounds whatever the input."""
    xyz = np.ascontiguousarray(xyz, dtype=np.float64)
    if xyz.ndim != 2 or xyz.shape[1] != 3:
        raise ValueError(f"fps_order: xyz must be [n, 3] (got {xyz.shape})")
    n, start, L = xyz.shape[0], int(start), int(L)
    if not (1 <= L <= n and 0 <= start < n):
        raise ValueError(f"fps_order: needs 1 <= L <= n and 0 <= start < n (got n = {n}, L = {L}, start = {start})")
    x, y, z = xyz[:, 0].copy(), xyz[:, 1].copy(), xyz[:, 2].copy()
    d = np.full(n, np.inf)
    order = np.empty(L, dtype=np.int64)
    s = start
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(L):
            order[k] = s
            if k + 1 == L:
                break
            d[s] = -1.0                    # r >= 0 or NaN: never below -1, a picked point stays picked
            dx, dy, dz = x - x[s], y - y[s], z - z[s]
            r = (dx * dx + dy * dy) + dz * dz
            np.copyto(d, r, where=r < d)
            s = int(np.argmax(d))          # the first of the largest: no d is a NaN
    return order


def fps_indices(seed_word, b, xyz, P):
    """int64 [P]: the rows sample `b` of a batch takes from the cloud xyz (float64 [n, 3]) under farthest-point sampling
    from fps_start(seed_word, b, n): idx[p] = order[p mod n], order = fps_order(xyz, start, min(n, P)) — a cloud shorter
    than P repeats its order cyclically (this sampler's `replace = n < P`).  1 <= n < 2^31, P >= 1."""
    xyz = np.asarray(xyz, dtype=np.float64)
    n, P = xyz.shape[0], int(P)
    if not (1 <= n < 1 << 31 and P >= 1):
        raise ValueError(f"fps_indices: needs 1 <= n < 2^31 and P >= 1 (got n = {n}, P = {P})")
    order = fps_order(xyz, fps_start(seed_word, b, n), min(n, P))
    return order[np.arange(P) % n]


# ---------------------------------------------------------------------------------------------------------------------
# The augmentation extension of the sampled forms (csrc/cloud.hip, the `_ext` entry points): a random scale, per-point
# jitter and random point dropout inside the gather — one launch, float64, one rounding — keyed like everything above.
# All float64, every operation rounded on its own (no fma).
#
#   ext [B, 8] float64 per sample {sx, sy, sz, sigma, clip, drop, 0, 0}: device memory BESIDE the parameter block
#   K = key 2^32 | key2, (key, key2) = sample_keys(seed_word, b)                       one per (seed word, sample)
#   dropped(p)   p >= 1 and (mix64(K ^ KEY_DROP, p) >> 11) 2^-53 < drop;  p_eff = 0 if dropped else p
#   row p        = the row p_eff of the plain form: source index idx(b, p_eff), then (xr, yr, z) by today's flips and
#                  z-rotation (today's bits), then
#   g_k          = float64(S_k - 131070) JITTER_C, S_k the sum of the four 16-bit fields of mix64(K ^ KEY_JITTER, 3 p_eff + k)
#   j_k          = min(max(sigma g_k, -clip), clip)                                    (a NaN sigma or clip gives NaN)
#   x' = xr sx + j_0, y' = yr sy + j_1, z' = z sz + j_2, rounded to fp32 once; sigma == 0 adds NOTHING (-0.0 keeps its sign)
#
# Jitter and dropout are keyed by word 0 of the seed words and the sample's LOCAL position b: like the row choice they
# are per (step, rank) and NOT world-size invariant.  The scales and the dropout ratio of a resident epoch
# (epoch_augment_ext) are keyed like the flips by (epoch, global slot) alone and ARE world-size invariant.
# Farthest-point sampling keeps measuring distance on the unscaled resident coordinates: an anisotropic scale is not an
# isometry, so the rows it takes are the farthest points of the cloud as it is stored, not as it is emitted.  Accepted.
# ---------------------------------------------------------------------------------------------------------------------
KEY_SCALE, KEY_DROPOUT = 0xA54FF53A5F1D36F1, 0x510E527FADE682D1          # per (epoch, global slot): + k for the axes
KEY_JITTER, KEY_DROP = 0x9B05688C2B3E6C1F, 0x1F83D9ABFB41BD6B            # per (seed word, sample, point)
JITTER_C = float.fromhex("0x1.bb67ae8584caap-16")                        # the double nearest to sqrt(3) 2^-16
JITTER_MAX = 131070 * JITTER_C                                           # 3.46405...: every |g| is at most this
EXT_IDENTITY = (1.0, 1.0, 1.0, 0.0, np.inf, 0.0, 0.0, 0.0)
_NO_AUGMENT = {"scale": (1.0, 1.0), "anisotropic": False, "jitter_sigma": 0.0, "jitter_clip": np.inf, "max_dropout": 0.0}


def check_augment(cfg):
    """The extension's configuration with every key present (a copy), or ValueError.  Keys, all optional, an absent one
    the identity: scale (lo, hi) finite with 0 < lo <= hi ((1, 1)); anisotropic (False: one scale for the three axes);
    jitter_sigma >= 0, finite (0); jitter_clip > 0, finite or inf (inf: no clip); max_dropout in [0, 1] (0).  None and {}
    mean no extension at all and return None."""
    if cfg is None or (isinstance(cfg, dict) and not cfg):
        return None
    if not isinstance(cfg, dict):
        raise ValueError(f"augment: must be a dict or None, got {type(cfg).__name__}")
    unknown = set(cfg) - set(_NO_AUGMENT)
    if unknown:
        raise ValueError(f"augment: unknown keys {sorted(unknown)} (known: {sorted(_NO_AUGMENT)})")
    c = dict(_NO_AUGMENT, **cfg)
    try:
        lo, hi = (float(v) for v in c["scale"])
    except (TypeError, ValueError):
        raise ValueError(f"augment: scale must be a pair (lo, hi), got {c['scale']!r}") from None
    if not (np.isfinite(lo) and np.isfinite(hi) and 0.0 < lo <= hi):
        raise ValueError(f"augment: scale needs finite 0 < lo <= hi, got ({lo}, {hi})")
    c["scale"] = (lo, hi)
    if not isinstance(c["anisotropic"], (bool, np.bool_)):
        raise ValueError(f"augment: anisotropic must be a bool, got {c['anisotropic']!r}")
    c["anisotropic"] = bool(c["anisotropic"])
    for key in ("jitter_sigma", "jitter_clip", "max_dropout"):
        if isinstance(c[key], (bool, np.bool_)):
            raise ValueError(f"augment: {key} must be a number, got {c[key]!r}")
        try:
            c[key] = float(c[key])
        except (TypeError, ValueError):
            raise ValueError(f"augment: {key} must be a number, got {c[key]!r}") from None
    if not (np.isfinite(c["jitter_sigma"]) and c["jitter_sigma"] >= 0.0):
        raise ValueError(f"augment: jitter_sigma must be finite and >= 0, got {c['jitter_sigma']}")
    if not c["jitter_clip"] > 0.0:
        raise ValueError(f"augment: jitter_clip must be > 0 (inf: no clip), got {c['jitter_clip']}")
    if not 0.0 <= c["max_dropout"] <= 1.0:
        raise ValueError(f"augment: max_dropout must be in [0, 1], got {c['max_dropout']}")
    return c


def augment_cfg8(cfg):
    """float64 [8] {lo, hi, anisotropic, sigma, clip, max_dropout, 0, 0}: what wf3d_cloud_epoch_params_ext takes (host
    memory) for a configuration (checked here)."""
    c = check_augment(cfg) or dict(_NO_AUGMENT)
    return np.array([c["scale"][0], c["scale"][1], 1.0 if c["anisotropic"] else 0.0, c["jitter_sigma"], c["jitter_clip"],
                     c["max_dropout"], 0.0, 0.0], dtype=np.float64)


def ext_draws(cfg):
    """(scale values, dropout ratios) one sample of a HOST-staged batch draws from np.random, in this order: 1 scale
    value (3 when anisotropic) when scale is not (1, 1), then 1 dropout ratio when max_dropout > 0."""
    c = check_augment(cfg) or dict(_NO_AUGMENT)
    return (0 if c["scale"] == (1.0, 1.0) else (3 if c["anisotropic"] else 1)), (1 if c["max_dropout"] > 0.0 else 0)


def ext_rows(cfg, u_scale, u_drop):
    """float64 [B, 8]: the extension rows of B samples from uniform draws in [0, 1) — u_scale [B, k], k = 0 (scale (1, 1)
    stays 1), 1 (one value for the three axes) or 3; u_drop [B] or None (drop = 0): s_k = lo + u_k (hi - lo),
    drop = u_drop max_dropout, sigma and clip copied."""
    c = check_augment(cfg) or dict(_NO_AUGMENT)
    lo, hi = (np.float64(v) for v in c["scale"])
    u = np.asarray(u_scale, dtype=np.float64)
    B = u.shape[0]
    ext = np.zeros((B, 8), dtype=np.float64)
    ext[:, :3] = lo + u.reshape(B, -1) * (hi - lo) if u.size else 1.0
    ext[:, 3], ext[:, 4] = c["jitter_sigma"], c["jitter_clip"]
    if u_drop is not None:
        ext[:, 5] = np.asarray(u_drop, dtype=np.float64) * np.float64(c["max_dropout"])
    return ext


def ext_row(cfg, u_scale=(), u_drop=None):
    """float64 [8]: ext_rows for one sample (u_scale of 0, 1 or 3 values, u_drop a value or None)."""
    return ext_rows(cfg, np.asarray(u_scale, dtype=np.float64).reshape(1, -1), None if u_drop is None else [u_drop])[0]


def _point_key(seed_word, b, salt):
    key, key2 = sample_keys([int(seed_word) & 0xFFFFFFFF], b)
    return ((int(key[0]) << 32) | int(key2[0])) ^ salt


def jitter_noise(seed_word, b, p):
    """float64 [len(p), 3] (or [3] for a scalar p): g of output row(s) p of sample b under `seed_word` — Irwin-Hall of four
    16-bit fields, centred and scaled: mean 0, variance 1 - 2^-32, |g| <= JITTER_MAX = 3.46405, excess kurtosis -0.3; no
    transcendental.  Per (seed word, LOCAL sample position, point): not world-size invariant."""
    pp = np.atleast_1d(np.asarray(p, dtype=np.int64))
    K = _point_key(seed_word, b, KEY_JITTER)
    ctr = (3 * pp[:, None] + np.arange(3, dtype=np.int64)[None, :]).reshape(-1)
    z = mix64(K, ctr)
    f = _u(0xFFFF)
    S = ((z & f) + ((z >> _u(16)) & f) + ((z >> _u(32)) & f) + (z >> _u(48))).astype(np.int64) - 131070
    g = (S.astype(np.float64) * JITTER_C).reshape(-1, 3)
    return g[0] if np.ndim(p) == 0 else g


def dropped(seed_word, b, p, drop):
    """bool [len(p)] (or a bool for a scalar p): output row p of sample b is dropped — it becomes an exact copy of output
    row 0 (PointNet++'s random_point_dropout): p >= 1 and (mix64(K ^ KEY_DROP, p) >> 11) 2^-53 < drop.  Row 0 never is;
    drop = 0 (or a NaN) drops nothing, drop = 1 every row p >= 1."""
    pp = np.atleast_1d(np.asarray(p, dtype=np.int64))
    u = (mix64(_point_key(seed_word, b, KEY_DROP), pp) >> _u(11)).astype(np.float64) * 2.0 ** -53
    with np.errstate(invalid="ignore"):
        d = (pp >= 1) & (u < np.float64(drop))
    return bool(d[0]) if np.ndim(p) == 0 else d


def effective_rows(seed_word, b, P, drop):
    """int64 [P]: p_eff of the P output rows of sample b — 0 for a dropped row, else p.  Everything behind (the source
    index idx(b, p_eff), the noise jitter_noise(., b, p_eff)) uses p_eff."""
    p = np.arange(int(P), dtype=np.int64)
    return np.where(dropped(seed_word, b, p, drop), 0, p)


def augment_point(xyz_rot, ext_row, noise):
    """float32 [..., 3]: (xr, yr, z) float64 — a row's first three columns behind today's flips and z-rotation, with
    today's bits — under ext_row = {sx, sy, sz, sigma, clip, drop, ..} and noise g [..., 3]:
    x' = xr sx + j_0, y' = yr sy + j_1, z' = z sz + j_2, j_k = min(max(sigma g_k, -clip), clip), every operation rounded
    on its own, the result rounded to fp32 once.  sigma == 0 adds nothing (-0.0 keeps its sign).  Columns 3 and up of a
    row are not the extension's."""
    e = np.asarray(ext_row, dtype=np.float64)
    v = np.asarray(xyz_rot, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        out = v * e[:3]
        if e[3] != 0.0:
            j = e[3] * np.asarray(noise, dtype=np.float64)
            out = out + np.minimum(np.maximum(j, -e[4]), e[4])
        return out.astype(np.float32)


def epoch_augment_ext(key, e, g, cfg):
    """float64 [len(g), 8]: the extension rows of the global slots g of epoch e, keyed like the flips by c = e 2^32 + g
    alone — world-size invariant: u_k = (mix64(key ^ (KEY_SCALE + k), c) >> 11) 2^-53, s_k = lo + u_k (hi - lo), k = 0, 1,
    2 when anisotropic, else k = 0 for the three axes; drop = u_d max_dropout from KEY_DROPOUT; sigma and clip copied."""
    cfg8 = augment_cfg8(cfg)
    lo, hi, aniso, sigma, clip, maxdrop = cfg8[:6]
    g = np.atleast_1d(np.asarray(g, dtype=np.int64))
    c = [((int(e) << 32) + int(k)) & _M64 for k in g]
    ext = np.zeros((g.size, 8), dtype=np.float64)

    def unit(salt):
        return (mix64(int(key) ^ (salt & _M64), c) >> _u(11)).astype(np.float64) * 2.0 ** -53
    for k in range(3):
        ext[:, k] = lo + unit(KEY_SCALE + (k if aniso else 0)) * (hi - lo)
    ext[:, 3], ext[:, 4] = sigma, clip
    ext[:, 5] = unit(KEY_DROPOUT) * maxdrop
    return ext
