"""tests/sx8_model.py, the integer model of the sx8 split (hi = bf16_rne(v), lo = bf16_rne(v - hi); include/wf3d.h),
held to torch's bfloat16 cast on the CPU, and the two constructions that test_sx8_producers_gpu.py relies on to ask
the kernels for exact bits:

  * the payload: a fixed table of fp32 patterns on which every rounding of the split is live.  Each class is counted
    from the model and must be present; the format's bound |v - hi - lo| <= 2^-17 |v| holds on all of it;
  * the exact LayerNorm input: rows of +-a (a a power of two, as many + as -) have mean 0 and variance a^2 in fp32 in
    any summation order, so with eps = 0 and beta = 0 a kernel must emit mu = 0, rs = 1/a and h = +-gamma, bit for bit.

Also the written record of one property the format does NOT have: splitting hi + lo again does not always give the same
two planes (when lo was rounded up onto half an ulp of an odd hi, the sum is a tie that goes to the even neighbour).
A kernel that moves an sx8 operand therefore has to move its planes, not re-split their sum."""
import numpy as np
import pytest
import torch

import helpers as H
import sx8_model as M


def torch_split(v):
    t = torch.from_numpy(np.ascontiguousarray(v))
    hi = t.bfloat16().float()
    return hi.numpy(), (t - hi).bfloat16().float().numpy()


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def test_model_equals_torch_on_payload_and_random_patterns():
    p, _ = M.payload()
    rng = np.random.default_rng(0)
    # 1e6 random patterns in range: any sign and mantissa, biased exponent 67 .. 186 (2^-60 <= |v| < 2^60)
    bits = (rng.integers(0, 2, 1_000_000, dtype=np.uint32) << np.uint32(31)) | \
           (rng.integers(67, 187, 1_000_000, dtype=np.uint32) << np.uint32(23)) | rng.integers(0, 1 << 23, 1_000_000, dtype=np.uint32)
    for v in (p, bits.view(np.float32)):
        assert np.all(np.abs(v) >= 2.0 ** -60) and np.all(np.abs(v) <= 2.0 ** 60)
        hi, lo = M.split(v)
        th, tl = torch_split(v)
        assert same_bits(hi, th) and same_bits(lo, tl)
        err = np.abs(v.astype(np.float64) - hi.astype(np.float64) - lo.astype(np.float64))
        assert np.all(err <= 2.0 ** -17 * np.abs(v.astype(np.float64)))


def test_every_rounding_class_is_in_the_payload():
    p, counts = M.payload()
    assert p.size == 2 * len(M.EXPONENTS) * len(M.HIGH_MANTISSAS) * len(M.LOW16)
    assert set(counts) == set(M.CLASSES)
    for k in M.CLASSES:
        assert counts[k] > 0, k
    # both signs of v inside every class, and a tile puts every class on every column of an sx8 group
    cls = M.classify(p.view(np.uint32))
    t = M.tile(64, 64)
    tc = M.classify(np.ascontiguousarray(t).view(np.uint32).reshape(-1))
    for k in M.CLASSES:
        assert (cls[k] & (p > 0)).any() and (cls[k] & (p < 0)).any(), k
        assert tc[k].reshape(64, 8, 8).any(axis=(0, 1)).all(), k


def test_pack_is_the_inverse_of_unpack():
    v = M.tile(5, 24, off=3)
    hi, lo = M.split(v)
    s = torch.from_numpy(M.pack(v))
    uh, ul = H.unpack_sx8(s)
    assert same_bits(uh.numpy(), hi) and same_bits(ul.numpy(), lo)
    ph, pl = M.planes16(s)
    assert torch.equal(ph, M.bits16(torch.from_numpy(hi))) and torch.equal(pl, M.bits16(torch.from_numpy(lo)))
    # layout: 8 high parts, then 8 low parts, per group of 8 columns
    raw = s.view(torch.bfloat16).float().numpy()
    assert same_bits(raw[:, 0:8], hi[:, 0:8]) and same_bits(raw[:, 8:16], lo[:, 0:8]) and same_bits(raw[:, 16:24], hi[:, 8:16])


def test_torch_integer_model_equals_numpy_model():
    v = M.tile(7, 40)
    hi, lo = M.split(v)
    th, tl = M.split_torch(torch.from_numpy(v))
    assert same_bits(th.numpy(), hi) and same_bits(tl.numpy(), lo)


def test_resplitting_the_sum_does_not_keep_the_planes():
    p, _ = M.payload()
    hi, lo = M.split(p)
    s = hi + lo                                                    # exact in fp32
    assert np.array_equal(s.astype(np.float64), hi.astype(np.float64) + lo.astype(np.float64))
    h2, l2 = M.split(s)
    moved = ~((h2.view(np.uint32) == hi.view(np.uint32)) & (l2.view(np.uint32) == lo.view(np.uint32)))
    assert moved.any()
    assert np.array_equal((h2 + l2)[moved], s[moved])             # the same value, held by other planes
    # every such element: lo went up onto half an ulp of an odd hi
    assert np.all(((hi.view(np.uint32) >> np.uint32(16)) & np.uint32(1))[moved] == 1)


@pytest.mark.parametrize("order", ["seq", "pair", "lanes"])
@pytest.mark.parametrize("D,a", [(8, 2.0), (136, 0.25), (1024, 0.25), (4088, 2.0 ** -5)])
def test_exact_layernorm_construction(order, D, a):
    R = 7
    s = M.signs(R, D)
    assert np.all(s.sum(axis=1) == 0) and np.all(np.abs(s) == 1)
    gamma = M.tile(1, D, off=11)[0]
    mean, rstd, h = M.ln_reference(s * np.float32(a), gamma, order)
    assert same_bits(mean, np.zeros(R, dtype=np.float32))
    assert same_bits(rstd, np.full(R, 1.0 / a, dtype=np.float32))
    assert same_bits(h, s * gamma[None, :])
