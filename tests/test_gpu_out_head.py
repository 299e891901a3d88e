"""-m gpu: ltrx_out_head_fwd (Linear(D, n_out) + activation + the sum over the output units, one launch, exact fp32) against a numpy
fp64 evaluation of the same fp32 inputs.  Inputs at the scale of a trained head: x ~ N(0, 1), W ~ N(0, 1) / sqrt(D), bias ~ N(0, 1), so
every pre-activation is of order 1.  Tolerance: ``close`` of tests/cases.py (1e-5 + 1e-5 |ref|) on ``out`` and ``score`` -- the bar of
the other fp32 contract tests; it holds at D = 1024, so the entrywise gamma_D bound the issue allows instead is not used."""
import functools

import numpy as np
import pytest
import torch

from tests.cases import close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS = 257                                                    # 1 and 5: fewer rows than a workgroup has waves; 257: the grid-stride wrap


@functools.lru_cache(maxsize=None)
def _inputs(D):
    """x [ROWS, D + 12] (the strided form reads its first D columns), W [8, D], bias [8] and their device copies; never modified"""
    rng = np.random.default_rng(D)
    x = rng.standard_normal((ROWS, D + 12)).astype(np.float32)
    W = (rng.standard_normal((8, D)) / np.sqrt(D)).astype(np.float32)
    b = rng.standard_normal(8).astype(np.float32)
    t = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
    return x, W, b, t(x), t(np.ascontiguousarray(x[:, :D])), t(W), t(b)


def _ref(x, W, b, act):
    z = x.astype(np.float64) @ W.astype(np.float64).T + b.astype(np.float64)
    p = 1.0 / (1.0 + np.exp(-z)) if act == 1 else z
    return p, p.sum(-1)


def _launch(x, W, b, rows, act, out=True, score=True):
    from allrank_amd import _lib as LB, kernels as KN
    o = torch.full((rows, W.shape[0]), float("nan"), device=DEV) if out else None
    s = torch.full((rows,), float("nan"), device=DEV) if score else None
    assert KN.out_head_fwd(LB.lib(), LB.stream_of(x), x, W, b, rows, act, o, s)
    torch.cuda.synchronize()
    return o, s


@pytest.mark.parametrize("n_out", [1, 2, 5, 8])
@pytest.mark.parametrize("D", [4, 36, 144, 260, 1024])
def test_out_and_score_equal_fp64_within_close(D, n_out):
    """D: one float4; fewer float4 than lanes; the shipped width; just over one float4 per lane; the cap.  Every row count, both
    activations, dense rows and rows of stride D + 12"""
    x, W, b, xs_d, xd_d, W_d, b_d = _inputs(D)
    for rows in (1, 5, ROWS):
        for act in (0, 1):
            p, s = _ref(x[:rows, :D], W[:n_out], b[:n_out], act)
            for xin in (xd_d, xs_d[:, :D]):
                o_d, s_d = _launch(xin, W_d[:n_out], b_d[:n_out], rows, act)
                err_o, err_s = np.abs(o_d.cpu().numpy() - p).max(), np.abs(s_d.cpu().numpy() - s).max()
                print("D %d n_out %d rows %d act %d stride %d: max err out %.3g score %.3g" % (D, n_out, rows, act, xin.stride(0), err_o, err_s))
                assert close(o_d.cpu().numpy(), p) and close(s_d.cpu().numpy(), s), (rows, act, xin.stride(0), err_o, err_s)


def test_either_output_alone_holds_the_same_bits():
    _, _, _, xs_d, _, W_d, b_d = _inputs(260)
    both = _launch(xs_d[:, :260], W_d[:5], b_d[:5], ROWS, 1)
    only_out = _launch(xs_d[:, :260], W_d[:5], b_d[:5], ROWS, 1, score=False)[0]
    only_score = _launch(xs_d[:, :260], W_d[:5], b_d[:5], ROWS, 1, out=False)[1]
    assert torch.equal(both[0], only_out) and torch.equal(both[1], only_score)


def test_results_do_not_depend_on_the_grid():
    """257 rows in one call == the same rows in two calls of 100 + 157, bit for bit"""
    _, _, _, _, xd_d, W_d, b_d = _inputs(144)
    o, s = _launch(xd_d, W_d[:5], b_d[:5], ROWS, 1)
    o1, s1 = _launch(xd_d, W_d[:5], b_d[:5], 100, 1)
    o2, s2 = _launch(xd_d[100:], W_d[:5], b_d[:5], 157, 1)
    assert torch.equal(o, torch.cat([o1, o2])) and torch.equal(s, torch.cat([s1, s2]))


def test_refusals():
    from allrank_amd import _lib as LB
    lib, P = LB.lib(), LB.ptr
    x, W, b = torch.zeros(4, 1040, device=DEV), torch.zeros(9, 1040, device=DEV), torch.zeros(9, device=DEV)
    o, s = torch.full((4, 9), 7.0, device=DEV), torch.full((4,), 7.0, device=DEV)
    call = lambda xp, D, n_out: lib.ltrx_out_head_fwd(xp, 1040, P(W), P(b), 4, D, n_out, 0, P(o), P(s), LB.stream_of(x))  # noqa: E731
    assert call(P(x), 144, 9) == -2 and call(P(x), 6, 2) == -2 and call(P(x), 1028, 2) == -2
    assert call(None, 144, 2) == -1
    torch.cuda.synchronize()
    assert (o == 7).all() and (s == 7).all()                 # a refused call writes nothing
