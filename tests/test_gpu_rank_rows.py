"""-m gpu: ltrx_rank_slates_rows_cu -- ltrx_rank_slates_cu with the sort key formed in the kernel from the packed output rows of a
model with n_out output units.  The rows are multiples of 1/64 in [0, 1], so every fp32 partial sum is exact and the expected order is
the stable descending sort of the exact sums (lower index first), with many exact ties by construction; ranked X (as bit patterns), y
and both tails must equal it exactly, from the padded grid and from a resident CSR set."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LENS = [0, 1, 2, 63, 64, 65, 256, 257, 1025]                  # tests/test_gpu_rank.py's: wave and workgroup edges, > 1 item per thread
CANARY = 0xDEADBEEF


def _batch(F, L):
    """sentinel features (every element its own bit pattern), labels that name (slate, item), and the same items as a CSR set"""
    B = len(LENS)
    cu = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int32)
    x = (np.arange(B * L * F, dtype=np.uint32) + np.uint32(0x3F800000)).reshape(B, L, F)
    y = np.arange(B, dtype=np.float32)[:, None] * 2048 + np.arange(L, dtype=np.float32)[None, :]
    for b, k in enumerate(LENS):
        y[b, k:] = -1
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    slates = types.SimpleNamespace(x_items=t(np.concatenate([x[b, :k] for b, k in enumerate(LENS)]).view(np.float32)),
                                   y_items=t(np.concatenate([y[b, :k] for b, k in enumerate(LENS)])), offsets=t(cu.astype(np.int64)))
    return B, cu, x, y, t, slates


def _canary(*shape):
    return torch.from_numpy(np.full(shape, CANARY, dtype=np.uint32).view(np.float32)).to(DEV)


@pytest.mark.parametrize("n_out", [1, 2, 5])
@pytest.mark.parametrize("F", [3, 8])
def test_ranked_slates_equal_the_stable_sort_of_the_exact_sums(F, n_out):
    from allrank_amd import _lib as LB, kernels as KN
    L = max(LENS) + 7
    B, cu, x, y, t, slates = _batch(F, L)
    out = np.random.default_rng(n_out).integers(0, 65, (int(cu[-1]), n_out)).astype(np.float32) / 64
    key = out.astype(np.float64).sum(-1)
    exp_x, exp_y, exp_p = np.zeros_like(x), np.full((B, L), -1, np.float32), np.zeros(int(cu[-1]), np.int32)
    for b, k in enumerate(LENS):
        o = np.argsort(-key[cu[b]:cu[b + 1]], kind="stable")
        exp_p[cu[b]:cu[b + 1]], exp_x[b, :k], exp_y[b, :k] = o, x[b, :k][o], y[b, :k][o]
    assert sum(len(np.unique(key[cu[b]:cu[b + 1]])) < k for b, k in enumerate(LENS) if k > 2) >= 5       # exact ties are there
    lib, out_d, cu_d = LB.lib(), t(out), t(cu)
    ids = torch.arange(B, dtype=torch.int64, device=DEV)
    got = []
    for src in (dict(x=t(x.view(np.float32)), y=t(y)), dict(slates=slates, ids=ids)):
        x_out, y_out, perm = _canary(B, L, F), _canary(B, L), torch.full((int(cu[-1]),), -7, dtype=torch.int32, device=DEV)
        KN.rank_slates_rows_cu(lib, LB.stream_of(x_out), out_d, cu_d, None, B, max(LENS), L, x_out, y_out, perm, **src)
        torch.cuda.synchronize()
        assert np.array_equal(perm.cpu().numpy(), exp_p)
        assert np.array_equal(x_out.cpu().numpy().view(np.uint32), exp_x) and np.array_equal(y_out.cpu().numpy(), exp_y)
        got.append((x_out, y_out, perm))
    if n_out == 1:                                            # the same bytes as ltrx_rank_slates_cu on the same scores
        x_out, y_out, perm = _canary(B, L, F), _canary(B, L), torch.full((int(cu[-1]),), -7, dtype=torch.int32, device=DEV)
        KN.rank_slates_cu(lib, LB.stream_of(x_out), out_d.view(-1), cu_d, None, B, max(LENS), L, x_out, y_out, perm, x=t(x.view(np.float32)), y=t(y))
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(got[0], (x_out, y_out, perm)))
