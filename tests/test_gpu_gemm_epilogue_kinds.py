"""The compile-time epilogue kinds of the 256-column NT kernel (allrank_amd/csrc/ltrx_gemm.hip, EPI_*), -m gpu.

The kernel picks a straight-line epilogue for the dropout-free launches of the default step (exact row tiles, three products, B read
as a pre-split image) and keeps the runtime-tested generic epilogue for everything else.  Which one ran must not show in a single bit:

  * forced tiles 6 / 7 / 8: bias, bias + ReLU and bias + residual launches equal the SAME tile's plain launch (no bias, act 0)
    followed by that arithmetic in torch fp32 on the device, and the plain launch over the image (straight-line kind) equals the plain
    launch over the fp32 operand (generic kind).  M = 512 is an exact tile count for all three heights (straight-line kinds with the
    image), M = 300 a ragged last tile that is no multiple of 64 either (generic kind); N = 512 gives two column tiles; K = 32 / 64 /
    96 / 160 are the prologue-only, tail-only, one-steady-iteration and several-iteration paths of the K loop.
  * the one-bit mask kinds, which exist on the automatic 256-row arm only (M = 21504, N = 512: 168 tiles): act 4 equals act 1, and
    act 5 fed with act 4's mask equals act 2 fed with act 1's output -- acts 1 / 2 run the generic epilogue.

The fp64 contract of the plain launch itself is tests/test_gpu_gemm_contract.py."""
import numpy as np
import pytest
import torch

from tests.test_gpu_gemm_contract import NT, _libs
from tests.test_gpu_parity import DEV

pytestmark = pytest.mark.gpu

N = 512
KS = (32, 64, 96, 160)


def _dev_view(win):
    """the window of a Win as a strided view of its device buffer"""
    return torch.as_strided(win.dev, (win.rows, win.cols), (win.ld, 1), win.off)


def _same_bits(a, b):
    return bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


@pytest.mark.parametrize("tile", [6, 7, 8])
def test_forced_tile_epilogues_equal_plain_launch_plus_torch_arithmetic(tile):
    for M in (512, 300):
        for K in KS:
            case = "kinds tile %d %dx%dx%d" % (tile, M, N, K)
            nt = NT(case, np.random.default_rng(100 * tile + K + M), M, N, K, K + 4, K + 8)
            bias_d = torch.as_tensor(nt.bias, device=DEV)
            aux_d = torch.as_tensor(nt.aux, device=DEV)

            def launch(act, bias, image):
                rc, c = nt.call(act, 0, tile, N + 4, 0.0, bias=bias, ldaux=N + 8, image=image)
                assert rc == 0, (case, act, bias, image, rc)
                c.fetch("%s act %d image %d" % (case, act, image))        # the NaN padding of ldc = N + 4 survives
                return _dev_view(c)

            generic_plain = launch(0, False, False)
            assert bool(torch.isfinite(generic_plain).all()), case
            for image in (False, True):
                plain = launch(0, False, image)
                assert _same_bits(plain, generic_plain), (case, "plain", image)
                with_bias = plain + bias_d
                assert _same_bits(launch(0, True, image), with_bias), (case, "bias", image)
                assert _same_bits(launch(1, True, image), torch.clamp_min(with_bias, 0.0)), (case, "bias + relu", image)
                assert _same_bits(launch(3, True, image), with_bias + aux_d), (case, "bias + residual", image)
            nt.inputs_unchanged()


@pytest.mark.parametrize("K", [32, 96])
def test_one_bit_mask_kinds_equal_the_generic_relu_epilogues(K):
    LB, lib = _libs()
    M, ldc = 21504, N + 4
    nbytes = lib.ltrx_gemm_nt_relu_bits_bytes(M, N, K)
    assert nbytes == 168 * 8192
    g = torch.Generator(device=DEV).manual_seed(7000 + K)
    a = torch.randn((M, K), device=DEV, generator=g)
    b = torch.randn((N, K), device=DEV, generator=g)
    bias = torch.randn((N,), device=DEV, generator=g)
    img = torch.empty_like(b)
    LB.check(lib.ltrx_split_image(LB.ptr(b), LB.ptr(img), b.numel(), None), "split_image")
    bits = torch.zeros(nbytes + 64, dtype=torch.uint8, device=DEV)
    bits[nbytes:] = 0xA5

    def launch(act, with_bias, aux, ldaux):
        c = torch.full((M, ldc), float("nan"), device=DEV)
        rc = lib.ltrx_gemm_nt(LB.ptr(a), K, LB.ptr(b), K, LB.ptr(img), LB.ptr(c), ldc, M, N, K, LB.ptr(bias) if with_bias else None, act,
                              LB.ptr(aux), ldaux, 0.0, 0, None, 0, 0, None)
        assert rc == 0, (act, rc)
        assert bool(torch.isnan(c[:, N:]).all()), act
        return c

    relu = launch(1, True, None, 0)                   # generic epilogue
    relu_bits = launch(4, True, bits, 0)              # straight-line, mask written
    assert bool((relu[:, :N] > 0).any()) and bool((relu[:, :N] == 0).any())
    assert _same_bits(relu_bits[:, :N], relu[:, :N])
    back = launch(2, False, relu, ldc)                # generic epilogue, saved activation read
    back_bits = launch(5, False, bits, 0)             # straight-line, mask read
    assert _same_bits(back_bits[:, :N], back[:, :N])
    assert bool((bits[nbytes:] == 0xA5).all())
