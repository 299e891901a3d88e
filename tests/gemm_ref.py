"""CPU reference of the split-bf16 GEMM arithmetic (allrank_amd/csrc/ltrx_gemm.hip)  --  TEST INFRASTRUCTURE, needs no GPU.

The kernels split every fp32 operand into bf16 terms while staging it (``split4<NTERMS>``) and issue bf16 x bf16 MFMAs with
fp32 accumulation (``mma_tile``).  A product of two bf16 values has 16 significand bits: it is exact in fp32 and in fp64.
``emulate_nt`` / ``emulate_tn`` therefore return, in fp64, the sum of EXACTLY the products a kernel issues; a correct kernel
differs from it only by its fp32 accumulation and its epilogue roundings, whatever the operands' scale.  That difference has an
a-priori bound (``bar_nt`` / ``bar_tn``), which is what tests/test_gpu_gemm_contract.py asserts entry by entry.
"""
import numpy as np
import torch

from oracle import dropout_oracle as D

U32 = 2.0 ** -24                     # unit round-off of fp32
U16 = 2.0 ** -8                      # unit round-off of bf16 (8 significand bits, round to nearest even)
PRODUCTS = {0: 3, 1: 6, 2: 1}        # precision code -> MFMA products per (a, b) pair
NTERMS = {0: 2, 1: 3, 2: 1}          # precision code -> bf16 terms per operand
# (term of A, term of B) of every product, as mma_tile / nt256_body / ltrx_gemm_tn256_kernel issue them
TERMS = {2: ((0, 0),),
         0: ((0, 1), (1, 0), (0, 0)),
         1: ((1, 1), (0, 2), (2, 0), (0, 1), (1, 0), (0, 0))}
# worst-case |a b - sum of the issued products| / |a b| (derived in tests/test_split_bf16_cpu.py)
SPLIT_BOUND = {2: 2 * U16 * (1 + U16), 0: 3 * U16 ** 2 * (1 + 2 * U16), 1: 4 * U16 ** 3 * (1 + 2 * U16)}


def bf16(x):
    """fp32 -> bf16 (round to nearest even) -> fp32"""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    return t.to(torch.bfloat16).to(torch.float32).numpy()


def split(x, n):
    """(hi, lo, lo2) as split4<n>: hi = bf16(x), lo = bf16(x - hi), lo2 = bf16((x - hi) - lo); lo2 is None for n < 3 (the
    kernels compute lo for n = 1 as well and do not use it).  The fp32 subtractions are exact."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        hi = bf16(x)
        r1 = x - hi
        lo = bf16(r1)
        lo2 = bf16(r1 - lo) if n == 3 else None
    return hi, lo, lo2


def _terms(x, prec):
    return [None if t is None else t.astype(np.float64) for t in split(x, NTERMS[prec])]


def emulate_nt(A, B, prec):
    """fp64 sum of the products ltrx_gemm_nt issues for C = A[M,K] B[N,K]^T at precision code ``prec``"""
    a, b = _terms(A, prec), _terms(B, prec)
    out = np.zeros((a[0].shape[0], b[0].shape[0]), np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for (ta, tb) in TERMS[prec]:
            out += a[ta] @ b[tb].T
    return out


def emulate_tn(A, B, prec):
    """fp64 sum of the products ltrx_gemm_tn issues for C = A[M,NP]^T B[M,KP]"""
    return emulate_nt(np.ascontiguousarray(np.asarray(A).T), np.ascontiguousarray(np.asarray(B).T), prec)


def abs_nt(A, B):
    """S = |A| |B|^T in fp64: the entrywise scale of every bound"""
    return np.abs(np.asarray(A, np.float64)) @ np.abs(np.asarray(B, np.float64)).T


def abs_tn(A, B):
    return np.abs(np.asarray(A, np.float64)).T @ np.abs(np.asarray(B, np.float64))


def epilogue64(acc, act, bias=None, aux=None, drop_p=0.0, seed=0, word=0):
    """fp64 form of the ltrx_gemm_nt epilogues 0 .. 3 on the accumulated products ``acc`` [M, N].  Returns (out, pre): ``pre``
    is acc + bias, the value whose sign the ReLU decides.  The dropout multipliers are the kernels' own counter-based mask
    (oracle/dropout_oracle.py, pinned to the kernels bit for bit), element index row * N + col, 1 / (1 - p) in fp32."""
    pre = acc + (0.0 if bias is None else np.asarray(bias, np.float64)[None, :])
    v = pre
    if act == 1:
        v = np.maximum(v, 0.0)
    if act == 2:
        inv_keep = np.float64(D.spec(drop_p, seed, word)[2]) if drop_p > 0 else 1.0
        v = np.where(np.asarray(aux) > 0, v * inv_keep, 0.0)
    elif drop_p > 0:
        v = v * D.keep_scale(drop_p, seed, word, v.shape).astype(np.float64)
    if act == 3:
        v = v + np.asarray(aux, np.float64)
    return v, pre


def bar_nt(S, K, prec, bias=None, aux=None):
    """entrywise bound on |kernel - epilogue64(emulate_nt)|: any-order fp32 summation of PRODUCTS * K exact products, plus the
    bias, dropout-scale and residual roundings: ((P K + 3) 2^-24) (S + |bias| + |aux|)"""
    s = np.array(S, np.float64, copy=True)
    if bias is not None:
        s = s + np.abs(np.asarray(bias, np.float64))[None, :]
    if aux is not None:
        s = s + np.abs(np.asarray(aux, np.float64))
    return (PRODUCTS[prec] * K + 3) * U32 * s


def bar_tn(S, M, prec):
    return (PRODUCTS[prec] * M + 3) * U32 * np.asarray(S, np.float64)


def bar_tn_bias(A, M):
    """bound on the bias gradient (fp32 column sums of A in any order, then the fixed-order slab sum)"""
    return (M + 2) * U32 * np.abs(np.asarray(A, np.float64)).sum(0)


def scaled_operands(rng, M, N, K, scaled=True, zero_rows=True):
    """A [M, K], B [N, K], N(0, 1); ``scaled``: rows of A and rows of B times 2^[-40, 40], columns of A times 2^[-6, 6] (features
    that are not normalised); one all-zero row in each (when it has more than one row)"""
    A = rng.standard_normal((M, K))
    B = rng.standard_normal((N, K))
    if scaled:
        A = A * 2.0 ** rng.integers(-40, 41, (M, 1)) * 2.0 ** rng.integers(-6, 7, (1, K))
        B = B * 2.0 ** rng.integers(-40, 41, (N, 1))
    A, B = A.astype(np.float32), B.astype(np.float32)
    if zero_rows:
        if M > 1:
            A[int(rng.integers(M))] = 0.0
        if N > 1:
            B[int(rng.integers(N))] = 0.0
    return A, B
