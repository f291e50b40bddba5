"""Properties of the split-GEMM arithmetic that hold across kernel forms (csrc/gemm_split.hip).

The persistent and the plain 256x256 forward kernel run the same slice pipeline: both accumulate the same MFMAs in the
same order from zero, so they must agree bit for bit.  The 256x128 wgrad form (gemm_split_dma3_kernel<true, NP>) is
held to exact integer results over one, two and three slices (the prologue and `ahead` edges of its three-stage
pipeline) and over a split-K launch with slabs, overwriting and accumulating.

fp64 references: products = 3 (bf16x3) is compared with the product of the fp32 operands; products = 1 (plain bf16 on
the hi planes) with the product of the hi planes read back from the sx8 operands — the arithmetic that mode defines
(tests/test_precision_bf16_gpu.py) — both within the 3e-5 of max |C| that tests/test_variants_gpu.py uses."""
import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu

TOL = 3e-5


def hi_plane(s):
    """fp64 hi plane of a contiguous sx8 matrix [R, C]: per 8 columns, the first 8 of 16 bf16 values."""
    R, C = s.shape
    return s.contiguous().view(torch.bfloat16).view(R, -1, 16)[:, :, :8].reshape(R, C).double()


@pytest.mark.parametrize("products", [3, 1])
@pytest.mark.parametrize("K", [256, 320])
def test_persistent_and_plain_256x256_same_bits(K, products):
    """192 tiles of 256x256: K is not split; the plain kernel runs when tiles < 2 x CUs, the persistent one under
    gemm_cus = 8 (192 >= 16).  K = 256 is 8 slices, the persistent form's minimum; K = 320 is 10."""
    from wf3d import ops
    dev = torch.device("cuda:0")
    M, N = 4096, 3072
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    assert (M // 256) * (N // 256) < 2 * cus, "default options would not select the plain kernel on this chip"
    g = torch.Generator(device=dev).manual_seed(K + products)
    A, B = torch.randn(M, K, device=dev, generator=g), torch.randn(N, K, device=dev, generator=g)
    As, Bs = ops.split_rows(A), ops.split_rows(B)
    plain = ops.gemm_split(As, Bs, products=products)
    with H.lib_option("gemm_cus", 8):
        persistent = ops.gemm_split(As, Bs, products=products)
    want = A.double() @ B.double().T if products == 3 else hi_plane(As) @ hi_plane(Bs).T
    scale = float(want.abs().max())
    e_plain = float((plain.double() - want).abs().max()) / scale
    e_pers = float((persistent.double() - want).abs().max()) / scale
    print(f"K={K} products={products}: plain {e_plain:.2e} persistent {e_pers:.2e} of max |C|")
    assert torch.equal(plain, persistent)
    assert e_plain < TOL and e_pers < TOL, (e_plain, e_pers)


def small_ints(shape, mul, mod):
    """integers in [-4, 4] (mod <= 9): exact in the bf16 hi plane"""
    n = 1
    for s in shape:
        n *= s
    return ((torch.arange(n, device="cuda:0") * mul) % mod - mod // 2).float().reshape(shape)


@pytest.mark.parametrize("products", [3, 1])
@pytest.mark.parametrize("Mo,No", [(256, 128), (512, 384)])
def test_256x128_wgrad_exact_on_integers(Mo, No, products):
    """|a|, |b| <= 4, K <= 4096: every product is exact and every sum stays below 4 * 4 * 4096 + 4 < 2^24, so the fp32
    accumulation, the split-K slabs and their combine are all exact whatever their order."""
    from wf3d import ops
    C0 = small_ints((Mo, No), 5, 9)
    for K in (32, 64, 96, 4096):
        A, B = small_ints((K, Mo), 7, 9), small_ints((K, No), 11, 7)
        As, Bs = ops.split_rows(A), ops.split_rows(B)
        assert ops.gemm_split_tn_ok(As, Bs)
        want = A.double().T @ B.double()
        got = ops.gemm_split_tn(As, Bs, products=products)
        assert torch.equal(got.double(), want), ("overwrite", K, Mo, No, float((got.double() - want).abs().max()))
        out = C0.clone()
        ops.gemm_split_tn(As, Bs, out=out, accumulate=True, products=products)
        assert torch.equal(out.double(), want + C0.double()), ("accumulate", K, Mo, No)
