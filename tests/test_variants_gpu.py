"""Every split-GEMM kernel forced onto every shape must stay correct: wf3d_set_option("split_kernel", v) with v = 3 (256x128
tiles: dma3 and the 256x128 wgrad kernel), 6 (the 256x256 forward / dgrad kernels) and 1 (the register-staged one)."""
import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kernel", [3, 6, 1])
def test_selectable_split_gemm_kernels(kernel):
    from wf3d import ops
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    worst = 0.0
    with H.lib_option("split_kernel", kernel):
        for M, N, K in [(256, 256, 32), (512, 384, 96), (1000, 200, 64), (2048, 512, 512)]:
            A, B, bias = torch.randn(M, K, device=dev), torch.randn(N, K, device=dev), torch.randn(N, device=dev)
            want = A.double() @ B.double().T + bias.double()
            got = ops.gemm_split(ops.split_rows(A), ops.split_rows(B), bias=bias)
            worst = max(worst, float((got.double() - want).abs().max() / want.abs().max()))
            Ai = (torch.arange(M * K, device=dev).reshape(M, K) % 9 - 4).float()
            Bi = (torch.arange(N * K, device=dev).reshape(N, K) % 5 - 2).float()
            gi = ops.gemm_split(ops.split_rows(Ai), ops.split_rows(Bi))
            assert torch.equal(gi.double(), Ai.double() @ Bi.double().T), ("integer data not exact", M, N, K)
        for K, Mo, No in [(64, 256, 256), (4096, 512, 256), (96, 256, 128)]:
            A, B = torch.randn(K, Mo, device=dev), torch.randn(K, No, device=dev)
            got = ops.gemm_split_tn(ops.split_rows(A), ops.split_rows(B))
            want = A.double().T @ B.double()
            worst = max(worst, float((got.double() - want).abs().max() / want.abs().max()))
    assert worst < 3e-5, (kernel, worst)
