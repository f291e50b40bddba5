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
