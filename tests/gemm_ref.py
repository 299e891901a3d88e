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


EUNSUPPORTED = -2
EPI_GENERIC, EPI_PLAIN, EPI_BIAS, EPI_RELU_BITS, EPI_MASK_READ, EPI_RESIDUAL = range(6)


def relu_bits_bytes_ref(M, N, K):
    if M <= 0 or N <= 0 or K <= 0 or N % 256 or K % 32:
        return 0
    t = -(-M // 256) * (N // 256)
    return t * 512 * 16 if (t >= 380 or 168 <= t <= 256) else 0


def nt_plan_ref(M, N, K, lda, ldb, ldc, act, has_bias, drop_on, prec, tile, vec_epi, bimg):
    """The dispatch of ltrx_gemm_nt as commit 5efdcb8 made it while launching, transcribed rule by rule from that source (it planned
    nowhere, and split rows by calling itself): the launches of a call whose pointers are valid, given its two alignment facts.
    Returns (rc, [(first row, rows, tile code, bf16 terms, tail, B image, epilogue kind), ...]); tile code 1-4 = the 128-column
    kernel actually run (precisions 1 and 2 have its 128x128x32 form only), 6 / 7 / 8 = the 256-column kernel."""
    if act in (4, 5) and (tile != 0 or prec == 1 or relu_bits_bytes_ref(M, N, K) == 0):
        return EUNSUPPORTED, []
    if (K & 3) or (lda & 3) or (ldb & 3) or lda < K or ldb < K or ldc < N:
        return EUNSUPPORTED, []
    if act in (4, 5) and (not vec_epi or K % 32):
        return EUNSUPPORTED, []
    plain, strict = prec == 2, prec == 1
    v = tile
    if v == 0 and not strict and N % 256 == 0 and K % 32 == 0 and vec_epi:
        nn = N // 256
        t = -(-M // 256) * nn
        if 256 < t < 380 and (not drop_on or act == 2) and nn <= 256:
            m1 = (256 // nn) * 256
            rc, first = nt_plan_ref(m1, N, K, lda, ldb, ldc, act, has_bias, drop_on, prec, 0, vec_epi, bimg)
            if rc:
                return rc, []
            rc, second = nt_plan_ref(M - m1, N, K, lda, ldb, ldc, act, has_bias, drop_on, prec, 0, vec_epi, bimg)
            return rc, [] if rc else first + [(m1 + s[0],) + s[1:] for s in second]
        t128 = -(-M // 128) * nn
        if t >= 360 or 168 <= t <= 256:
            v = 6
        elif 136 <= t < 168 and t128 > 256:
            v = 6
        elif 176 <= t128 <= 256:
            v = 7
        elif t128 < 176 and 176 <= -(-M // 64) * nn <= 512:
            v = 8
    if v == 0:
        v = 1
    if act in (4, 5) and v != 6:
        return EUNSUPPORTED, []
    if v in (6, 7, 8):
        if N % 256 or K % 32 or strict or not vec_epi or (v == 8 and act in (4, 5)):
            return EUNSUPPORTED, []
        tail = M % {6: 256, 7: 128, 8: 64}[v] != 0
        epi = EPI_GENERIC
        if not (drop_on or tail or plain or not bimg):
            epi = {0: EPI_BIAS if has_bias else EPI_PLAIN, 3: EPI_RESIDUAL if has_bias else EPI_GENERIC,
                   4: EPI_RELU_BITS if has_bias else EPI_GENERIC, 5: EPI_GENERIC if has_bias else EPI_MASK_READ}.get(act, EPI_GENERIC)
        if epi in (EPI_RELU_BITS, EPI_MASK_READ) and v != 6:           # (no such instantiation)
            return EUNSUPPORTED, []
        return 0, [(0, M, v, 1 if plain else 2, int(tail), int(bool(bimg)), epi)]
    if strict:
        return 0, [(0, M, 1, 3, 0, 0, EPI_GENERIC)]
    if plain:
        return 0, [(0, M, 1, 1, 0, 0, EPI_GENERIC)]
    return 0, [(0, M, v if v in (2, 3, 4) else 1, 2, 0, 0, EPI_GENERIC)]


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
