"""Integer model of the sx8 split (include/wf3d.h, csrc/split.hip) and the inputs that make its producers exact.

TEST INFRASTRUCTURE ONLY.  The format: every group of 8 fp32 columns is stored as 8 bf16 high parts followed by 8 bf16
low parts, hi = bf16_rne(v), lo = bf16_rne(v - hi).  This module states that on integer bit patterns in numpy, with no
floating-point cast of its own:

    rne_bits(bits)            fp32 bits -> bits of the nearest-even bfloat16 (low 16 bits zero)
    split(v)                  float32 array -> (hi, lo) float32 arrays
    pack(v) / pack_planes     the sx8 container (float32 [R, C]) of a matrix: the inverse of helpers.unpack_sx8
    split_torch(v)            the same split in torch integer ops, for matrices that should not leave the device
    payload()                 a fixed table of fp32 values on which every rounding of the split is live, with the
                              count of each rounding class — counted from this model
    tile(R, C, off)           the payload laid over a matrix with a per-row rotation
    signs(R, D) / ln_rows     rows of +-a with a zero sum: LayerNorm input whose statistics are exact in fp32

Range: 2^-60 <= |v| <= 2^60.  No bf16 subnormal, overflow or non-finite value occurs; those are out of scope here.
"""
import numpy as np
import torch

_U32, _U64 = np.uint32, np.uint64


def rne_bits(bits):
    """hi = ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16) << 16 on uint32 patterns (evaluated in 64 bits: no wrap)."""
    b = np.asarray(bits).astype(_U64)
    return ((((b + _U64(0x7FFF) + ((b >> _U64(16)) & _U64(1))) >> _U64(16)) << _U64(16)) & _U64(0xFFFFFFFF)).astype(_U32)


def split_bits(bits):
    """(hi_bits, lo_bits) of fp32 patterns: lo is the same rounding of the fp32 difference v - hi (exact in fp32)."""
    bits = np.ascontiguousarray(bits, dtype=_U32)
    hi = rne_bits(bits)
    r = bits.view(np.float32) - hi.view(np.float32)
    return hi, rne_bits(np.ascontiguousarray(r).view(_U32))


def split(v):
    """float32 array -> (hi, lo) float32 arrays of the same shape."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    hi, lo = split_bits(v.view(_U32))
    return hi.view(np.float32), lo.view(np.float32)


def pack_planes(hi, lo):
    """(hi, lo) float32 [R, C] holding bf16 values -> the sx8 container, float32 [R, C]."""
    R, C = hi.shape
    assert C % 8 == 0
    h = (np.ascontiguousarray(hi, dtype=np.float32).view(_U32) >> _U32(16)).astype(np.uint16).reshape(R, C // 8, 1, 8)
    l = (np.ascontiguousarray(lo, dtype=np.float32).view(_U32) >> _U32(16)).astype(np.uint16).reshape(R, C // 8, 1, 8)
    return np.ascontiguousarray(np.concatenate([h, l], axis=2)).reshape(R, 2 * C).view(np.float32).reshape(R, C)


def pack(v):
    """float32 [R, C] -> its sx8 container."""
    return pack_planes(*split(v))


def split_torch(v):
    """The split of a float32 tensor in torch integer arithmetic (any device): (hi, lo) float32 tensors."""
    def rne(t):
        b = t.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
        h = (((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16) & 0xFFFFFFFF
        h = torch.where(h >= 0x80000000, h - 0x100000000, h)
        return h.to(torch.int32).view(torch.float32)
    hi = rne(v)
    return hi, rne(v - hi)


def planes16(t):
    """sx8 tensor [R, C] -> (hi, lo) int16 tensors [R, C] of the raw bf16 bits."""
    R, C = t.shape
    b = t.contiguous().view(torch.int16).reshape(R, C // 8, 2, 8)
    return b[:, :, 0, :].reshape(R, C), b[:, :, 1, :].reshape(R, C)


def bits16(f):
    """float32 tensor holding bf16 values -> int16 tensor of the bf16 bits."""
    return (f.contiguous().view(torch.int32) >> 16).to(torch.int16)


# ---- the payload -------------------------------------------------------------------------------------------------
EXPONENTS = (-40, -17, -1, 0, 1, 13, 40)
HIGH_MANTISSAS = (0x00, 0x01, 0x2A, 0x55, 0x7E, 0x7F)       # even, odd, all-ones (a round-up carries into the exponent)
# low 16 bits: exact, just above, just below / on / just above the tie in hi, just below the next value; residuals with
# more than 8 significant bits; ties of the LOW part's own rounding (8 kept bits, then exactly one half): onto an even
# (0x4040) and an odd (0x40C0) kept mantissa, and the same two below the next bf16 value (negative residuals)
LOW16 = (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF, 0x1234, 0x5A5B, 0xA5A5, 0x4040, 0x40C0, 0xBFC0, 0xBF40, 0x7FC1)
CLASSES = ("lo_zero", "hi_tie_even", "hi_tie_odd", "hi_carry", "lo_opposite_sign", "lo_inexact", "lo_tie")


def classify(bits):
    """{class: bool mask} of fp32 patterns, from the model alone."""
    bits = np.ascontiguousarray(bits, dtype=_U32)
    hi, lo = split_bits(bits)
    v = bits.view(np.float32)
    r = np.ascontiguousarray(v - hi.view(np.float32)).view(_U32)
    tie = (bits & _U32(0xFFFF)) == _U32(0x8000)
    odd = ((bits >> _U32(16)) & _U32(1)) == _U32(1)
    lo_nz = (lo & _U32(0x7FFFFFFF)) != 0
    exact = hi.view(np.float32).astype(np.float64) + lo.view(np.float32).astype(np.float64) == v.astype(np.float64)
    return {
        "lo_zero": ~lo_nz,
        "hi_tie_even": tie & ~odd,                 # the truncated mantissa is even: the tie stays
        "hi_tie_odd": tie & odd,                   # it is odd: the tie goes up to the even neighbour
        "hi_carry": (hi >> _U32(23)) != (bits >> _U32(23)),
        "lo_opposite_sign": lo_nz & ((lo >> _U32(31)) != (bits >> _U32(31))),
        "lo_inexact": ~exact,
        "lo_tie": (r & _U32(0xFFFF)) == _U32(0x8000),
    }


_payload = None


def payload():
    """(values float32 [P], {class: count}).  The low-16 pattern varies fastest, so that neighbours differ in class."""
    global _payload
    if _payload is None:
        out = []
        for sign in (0, 1):
            for e in EXPONENTS:
                for m in HIGH_MANTISSAS:
                    for low in LOW16:
                        out.append((sign << 31) | ((e + 127) << 23) | (m << 16) | low)
        bits = np.array(out, dtype=_U32)
        _payload = (bits.view(np.float32).copy(), {k: int(m.sum()) for k, m in classify(bits).items()})
    return _payload


ROT = 13          # odd, and prime to len(LOW16): the classes walk over all 8 positions of a group from row to row


def tile(R, C, off=0):
    """float32 [R, C]: element (r, c) is payload[(c + ROT * r + off) mod P]."""
    p, _ = payload()
    idx = (np.arange(C, dtype=np.int64)[None, :] + ROT * np.arange(R, dtype=np.int64)[:, None] + off) % p.size
    return p[idx]


# ---- LayerNorm inputs with exact statistics -----------------------------------------------------------------------
def signs(R, D):
    """float32 [R, D] of +-1, every row summing to zero: square waves of period 2, 4 and 8 (all divide D, D % 8 == 0)
    shifted by the row index, so a row's + and - fall on different columns from row to row."""
    assert D % 8 == 0
    r = np.arange(R, dtype=np.int64)[:, None]
    k = np.array([1, 2, 4], dtype=np.int64)[r % 3]
    c = np.arange(D, dtype=np.int64)[None, :]
    return np.where(((c + r) // k) % 2 == 0, 1.0, -1.0).astype(np.float32)


def act_np(act, y):
    """act 0: identity, 1: ReLU (the two exact ones)."""
    return np.maximum(y, np.float32(0)) if act == 1 else y


def ln_reference(z, gamma, order):
    """LayerNorm(z) * gamma with eps = 0 and beta = 0 in plain fp32, the two row sums taken in the given order:
    'seq' left to right, 'pair' numpy's pairwise sum, 'lanes' 64 strided partial sums met in a butterfly."""
    z = np.asarray(z, dtype=np.float32)
    R, D = z.shape

    def rsum(a):
        if order == "seq":
            s = np.zeros(R, dtype=np.float32)
            for c in range(D):
                s = s + a[:, c]
            return s
        if order == "pair":
            return a.sum(axis=1, dtype=np.float32)
        lanes = np.zeros((R, 64), dtype=np.float32)
        for c0 in range(0, D, 4):
            lane = (c0 // 4) % 64
            for j in range(4):
                lanes[:, lane] = lanes[:, lane] + a[:, c0 + j]
        w = 64
        while w > 1:
            w //= 2
            lanes = lanes[:, :w] + lanes[:, w:2 * w]
        return lanes[:, 0]
    mean = rsum(z) / np.float32(D)
    d = z - mean[:, None]
    rstd = np.float32(1) / np.sqrt(rsum(d * d) / np.float32(D) + np.float32(0))
    return mean, rstd, d * rstd[:, None] * np.asarray(gamma, dtype=np.float32)[None, :]
