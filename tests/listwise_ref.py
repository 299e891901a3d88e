"""fp64 references, a-priori entrywise bars, fp32 transcriptions and the case table of the four listwise loss kernels
(allrank_amd/csrc/ltrx_listnet.hip, ltrx_listmle.hip, ltrx_approxndcg.hip, ltrx_lambdaloss.hip + the helpers of ltrx_device.h)
--  TEST INFRASTRUCTURE, plain numpy, needs no GPU.

As in tests/layernorm_ref.py every loss has functions that take the fp32 operands exactly as the kernel receives them (a Batch: the
padded grid [B, L] with the pad label, or the packed rows with cu_seqlens and an optional slate_order):

    *_ref   the operation in fp64, eps / alpha / sigma / mu the fp32 values widened; one slate at a time and, for the pair losses,
            in row chunks of CHUNK items, so that L = 6785 never needs an L x L matrix.  It returns every output (loss, per-slate
            values, gradient, lambdaLoss's pair count and order, listMLE's order), per entry the sum of the absolute values of its
            summands, and the propagated-error sums the bar needs.  tests/test_listwise_ref_cpu.py holds it to oracle/ltr_oracle.py
            (dtype=np.float64) on the padded grid: the oracle works in sorted space on [B, L, L] arrays, the reference in item order.
    *_bar   the bound on |kernel - *_ref| per entry: (fp32 roundings on the longest path) * u * (sum of |terms|) + the propagated
            error of what the entry depends on; gam(k) = k u / (1 - k u), u = 2^-24 (tests/step_ref.py).  No measured number.
    *_f32   the kernel's arithmetic in np.float32 in the operation order of the source, with ``wrong=`` one-line defects.

Accuracies the bars rest on and that are documented, not verified here: expf / logf / exp2f / log2f at 1 ulp (P_LIBM = 2 in units of u,
tests/step_ref.py), the hardware exp2 and rcp behind sigmoid_neg_fast at 1 ulp each (P_HW, the allowance of tests/attention_ref.py),
exp2f(0) = 1 exactly (so a label 0 has gain 0 exactly and an all-zero slate a dsum of exactly 0).  Division is the correctly rounded
one; a fused multiply-add only removes a rounding.  A result below FLT_MIN has no relative precision (flushed or denormal): the
exponentials of listNet and listMLE carry FLT_MIN absolutely.

The chains (k = roundings on the longest path of a sum; the first addition to 0.f is exact and still counted)
    quarter walk     thread (i, q) adds its partners j in [q lq, min(n, q lq + lq)), lq = (n + 3) >> 2, serially: lq additions
                     (lambdaLoss with ndcgLoss1 adds two terms per partner: 2 lq)
    combine          (p0 + p1) + (p2 + p3): 2                                                  k_pair(n) = lq + 2
    block_sum        a thread's own serial additions m, the 6 levels of wave_sum, the blockDim / 64 wave partials added in order
                                                                                               k_block(m, T) = m + 6 + T / 64
    block_inclusive_scan   a thread's chunk c = ceil(n / T) serially, the 6 shuffle steps of the wave scan, the wave offsets
                     (T / 64 - 1), `a[i] += base` (1)                                          k_scan(n, T) = c + 6 + T / 64
                     The exclusive prefix of a lane is the inclusive one of the lane below, so every entry is a sum of positive terms
                     with an error relative to ITSELF.  (Until this table existed it was `inc - tot`, a difference rounded at the size
                     of the scan value at the END of the thread's chunk: with c >= 2 -- ListMLE at L = 257 .. 512 and L > 1024 -- an
                     entry far below its chunk's end, the tail of a slate at score scale 30, lost all precision: C + eps off by a
                     factor.  The defect model "scan_base_by_subtraction" is that code.)

ListNet (256 threads).  e_i = expf(s_i - smax): the subtraction moves the argument by u |x_i|, so de_i = expm1(u |x_i|) (1 + P u) + P u
  relatively, + FLT_MIN; ssum: k_block(ceil(n / 256), 256) on positive terms; 1 / ssum 1; P_i = e_i inv_s 1:
      dP_i = comp(de_i, quot(max de, gam(k)), gam(2)) relatively, + 2 FLT_MIN;     T_i the same from the labels
  P + eps: (dP + u) relatively (both terms positive); logf: |log(1 + rho)| and P u |log|; T log(P + eps): T's error and 1; lsum
  k_block.  r_i = P / (P + eps): quot(dP, dP + u) and 1; T r: 1; rsum k_block.  Entry fl(fl(P rsum - T r) inv_div): the propagated
  P d_rsum + dP rsum + d(T r), the subtraction u on |P rsum| + |T r| -- the entry cancels, the bar is on that sum --, 1 / divisor and
  the product gam(2).  `P > 0` differs between fp32 and fp64 only where P < FLT_MIN; there the FLT_MIN terms (FLT_MIN / eps in r)
  cover both sides.  `T > 0` and `ssum > 0` are exact for labels 0..4 (asserted: a valid slate has e = 1 at its maximum).  A padded
  entry is P = T = 0: exactly 0.

ListMLE (256 threads, 1024 for L > 512).  The counting rank, the order and the arg-max (the first sorted position holding the exact
  fp32 maximum) involve no arithmetic: exact, compared bit for bit.  e_r as in ListNet; C_r (suffix sums: the scan of the reversed
  array): dC_r = sum_{r' >= r} e de + gam(k_scan) (C_r + that).  obs_r =
  logf(C + eps) - xm_r: (dC + u (C + eps)) / (C + eps) through the log, P u |log|, u |xm| of the subtraction x - xmax, u |obs|; lsum
  k_block(ceil(L / T), T).  q_r = 1 / (C + eps): quot(0, that) and 1; Q_r its prefix scan, as C.  g_r = fl(e_r Q_r - 1): e Q comp(de,
  dQ / Q, u) + u |g|; gsum k_block over |g| (+ dg).  Entry fl(g inv_div), at the arg-max fl(fl(g - gsum) inv_div): dg + d_gsum + u (|g|
  + |gsum|), gam(2).  Padded entries are written as 0.f.

ApproxNDCG (1024 threads).  gain = exp2f(y) - 1: P u 2^y + u gain; log2f(2 + rank) P u, the division 1; dsum k_block(ceil(n / 256),
  1024) on positive terms: dM relatively; maxDCG = fmaxf(dsum, eps) (dsum is 0 exactly or far above eps: asserted).  It is shared by
  the slate: G_i = gain / maxDCG carries quot(dgain, dM) and 1 into every entry.
  sg = rcp(1 + exp2(z log2 e)), z = alpha (s_i - s_j): the difference, two products and the constant move the argument by gam(4) |z|:
      dE = expm1(gam(4) |z|) (1 + P_HW u) + P_HW u;   1 + E: dE E / (1 + E) = dE (1 - sg), and u;  rcp P_HW u:
      dsg = comp(dE (1 - sg), u, P_HW u) relatively -- 3 u at sg -> 1, where it is an ABSOLUTE 3 u on 1 - sg
  pos_i = 1 + sum fmaxf(sg, eps): positive terms, k_pair + 1;  aD = log2f(1 + pos) >= 1: rho = d_pos / (1 + pos) + u through the log
  (rho / (ln 2 (1 - rho))) and P u aD;  v_i = G / aD 1; vsum k_block.  w_i = G / (aD aD (1 + pos) ln 2): 2 daD + rho + gam(4), 1.
  Pass 2 forms sigmoid(+z) as 1 - sg: e1 = sg dsg + FLT_MIN (below FLT_MIN fp32 has no relative precision; the product too), e2 = e1 +
  u (1 - sg + e1) absolutely, d_ds = (sg + e1)(1 - sg + e2)(1 + u) - ds.
  The term ds (a - c) carries d_ds (w_j + w_k) with the UNCLAMPED weights: `1 - sg >= eps` is decided in fp32 on a multiple of 2^-24,
  so it is `1 - sg != 0`, and wherever it differs from the fp64 decision the true 1 - sg is below e2 (fp32 says 0) or below eps (fp64
  says clamped, then ds < eps is added): the jump is inside d_ds (w_j + w_k) + ds w_j.  A band for it would span the whole saturated
  range (3 u >> eps), so this decision has no guard; the bar covers both sides.  + (ds + d_ds)(dw_j + dw_k), the subtraction and the
  product 2 u.  Entry fl(fl(alpha sum) inv_div): k_pair + 3 on sum |ds a| + |ds c|.

LambdaLoss (1024 threads).  Ranks, the pair count (sums of 1.f below 2^24) and the order are exact.  invD[p] = 1 / log2f(1 + p): dD =
  comp(P u, u).  maxDCG@k: gain invD, 1, k_block(ceil(n / 256), 1024); G as above.  Weights (w, dw absolutely) per scheme: ndcgLoss1 G
  invD; del = |invD[d] - invD[d + 1]|: dD (invD[d] + invD[d + 1]) + u del; |Ga - Gb|: dGa + dGb + u |.|; products 1 each; ndcgLoss2PP
  mu (del dg) + lr dg: 2 more; the label differences 1 (+ 1 per square).
  sig = 1 / (1 + expf(-dx)), dx = sigma (s_i - s_j): gam(2) |dx|, dE = expm1(gam(2) |dx|)(1 + P u) + P u, dsig = comp(dE (1 - sig), u,
  u); logf(q): dsig / (1 - dsig) + P u |log q| (q = eps: P u |ln eps|);  wl = w log q: dw |log q| + (w + dw) dlog + u |wl|;  l =
  fmaxf(wl, ln_eps) inv_lnb: max is 1-Lipschitz in both arguments: max(d_wl, P u |ln eps|), gam(2).  lsum: a thread's ceil(n / 256)
  lq (2 lq) additions, k_block.  g = w sigma (1 - sig) inv_lnb with 1 - sig a subtraction: sig dsig + u (1 - sig) ABSOLUTELY -- both
  orientations are evaluated from their own expf, so this holds for (i, j) and (j, i) alike --, gam(4).  Entry: k_pair on sum |g_ij| +
  |g_ji|; mean: 1 / div and the scaling product, gam(2); loss -a / div: k_block(1, 256) and 1.

Branch guard (a condition on the inputs, not a tolerance).  Where fp32 and fp64 could fall on different sides of `sig >= eps`,
`wl >= ln_eps` (lambdaLoss; the latter matters only where sig >= eps: below, the gradient is 0 either way and fmaxf is continuous),
`sg >= eps` (approxNDCG) the gradient jumps.  Every case keeps |quantity - threshold| > 2 x (the quantity's bound above); `inputs`
redraws the score of an offending item from the case's own stream, at most REPAIR_ROUNDS times, and *_ref asserts that none is left.
Exact ties (dx = 0) are far from every threshold.  No entry is left out of any comparison.
"""
import functools
import os
import re
from collections import namedtuple

import numpy as np

from oracle import ltr_oracle as O
from tests.step_ref import F, FLT_MIN, ONE, P_LIBM, U, _wave_sum, f64, gam, over, w, worst  # noqa: F401  (re-exported)

P_HW = 2.0                    # the hardware exp2 / rcp: 1 ulp <= 2 u (tests/attention_ref.py)
PAD = F(-1.0)
CHUNK = 512
REPAIR_ROUNDS = 8
LN2, LOG2E = float(np.log(2.0)), 1.4426950408889634
SCHEMES = O.LAMBDA_SCHEMES
ALL_PAIRS = 1                 # LTRX_SCHEME_NDCGLOSS1

# restated from the sources; tests/test_listwise_ref_cpu.py holds them to the text (source_constants)
NARR = dict(listnet=(2, 0), listmle=(6, 0), approxndcg=(7, 0), lambdaloss=(13, 2))
LDS_BUDGET = 160 * 1024 - 1024
DEFAULT_DYN_LDS = 48 * 1024
MAX_LONG = 16384


def block_threads(loss, L):
    return {"listnet": 256, "approxndcg": 1024, "lambdaloss": 1024, "listmle": 1024 if L > 512 else 256}[loss]


def source_constants():
    """the same numbers read from the source text"""
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "allrank_amd", "csrc")
    rd = lambda f: open(os.path.join(here, f)).read()     # noqa: E731
    dev = rd("ltrx_device.h")
    out = dict(narr={})
    for loss, f, var in (("listnet", "ltrx_listnet.hip", "listnet_arrays"), ("listmle", "ltrx_listmle.hip", "listmle_arrays"),
                         ("approxndcg", "ltrx_approxndcg.hip", "approx_arrays"), ("lambdaloss", "ltrx_lambdaloss.hip", "lambda_arrays")):
        m = re.search(r"static LtrxSlateArrays %s\{(\d+), (\d+), \w+\};" % var, rd(f))
        out["narr"][loss] = (int(m.group(1)), int(m.group(2)))
    m = re.search(r"#define LTRX_LDS_ARRAY_BUDGET_BYTES \((\d+) \* 1024 - (\d+)\)", dev)
    out["budget"] = int(m.group(1)) * 1024 - int(m.group(2))
    out["default_lds"] = int(re.search(r"#define LTRX_DEFAULT_DYNAMIC_LDS_BYTES \((\d+) \* 1024\)", dev).group(1)) * 1024
    assert re.search(r"bool in_lds\(int L\) const \{ return lds_bytes\(L\) <= \(size_t\)LTRX_LDS_ARRAY_BUDGET_BYTES; \}", dev)
    assert re.search(r"size_t floats\(int L\) const \{ return \(size_t\)narr \* \(size_t\)L \+ \(size_t\)extra_floats; \}", dev)
    assert re.search(r"if \(lds > LTRX_DEFAULT_DYNAMIC_LDS_BYTES\)", dev)
    assert re.search(r"size_t ws_stride\(int L\) const \{ return \(floats\(L\) \+ 3\) & ~\(size_t\)3; \}", dev)
    assert re.search(r"lambda_per_floats\(int B\) \{ return \(\(size_t\)\(2 \* B \+ 4\) \+ 3\) & ~\(size_t\)3; \}", rd("ltrx_lambdaloss.hip"))
    assert re.search(r"ltrx_per_slate_floats\(int B\) \{ return \(\(size_t\)B \+ 3\) & ~\(size_t\)3; \}", dev)
    m = re.search(r"const dim3 block\(L > (\d+) \? (\d+) : (\d+)\);", rd("ltrx_listmle.hip"))
    out["threads"] = dict(listmle=tuple(int(v) for v in m.groups()),
                          listnet=sorted(set(re.findall(r"dim3\((\d+)\), per, s", rd("ltrx_listnet.hip")))),
                          approxndcg=sorted(set(re.findall(r"dim3\((\d+)\), per, s", rd("ltrx_approxndcg.hip")))),
                          lambdaloss=sorted(set(re.findall(r"dim3\((\d+)\), per_loss, s", rd("ltrx_lambdaloss.hip")))))
    hdr = open(os.path.join(here, "..", "..", "include", "ltrx.h")).read()
    out["max_long"] = int(re.search(r"#define LTRX_MAX_LONG_SLATE_LEN (\d+)", hdr).group(1))
    return out


def lds_bytes(loss, L):
    narr, extra = NARR[loss]
    return (narr * L + extra) * 4


def in_lds(loss, L):
    """LtrxSlateArrays::in_lds restated: the arm (LDS / GWS) a length selects"""
    return lds_bytes(loss, L) <= LDS_BUDGET


def opts_in(loss, L):
    """the LDS launch asks for more than the default allowance"""
    return in_lds(loss, L) and lds_bytes(loss, L) > DEFAULT_DYN_LDS


def last_lds(loss, budget=LDS_BUDGET):
    narr, extra = NARR[loss]
    return (budget // 4 - extra) // narr


def per_floats(loss, B):
    return ((2 * B + 4 if loss == "lambdaloss" else B) + 3) & ~3


def workspace_bytes(loss, B, L):
    narr, extra = NARR[loss]
    stride = (narr * L + extra + 3) & ~3
    return (per_floats(loss, B) + (0 if in_lds(loss, L) else stride * B)) * 4


def comp(*rel):
    """(1 + a)(1 + b) ... - 1"""
    p = 1.0
    for r in rel:
        p = p * (1.0 + r)
    return p - 1.0


def quot(a, b):
    """(1 + a) / (1 - b) - 1"""
    return (1.0 + a) / (1.0 - b) - 1.0


def k_pair(n, two=False):
    return ((n + 3) >> 2) * (2 if two else 1) + 2


def k_block(m, T):
    return m + 6 + T // 64


def k_scan(n, T):
    return -(-n // T) + 6 + T // 64


# ---------------------------------------------------------------------------------------------------------------------------------
# batches: the two layouts behind one list of slates
# ---------------------------------------------------------------------------------------------------------------------------------
class Batch(object):
    """padded: s, y [B, L]; ragged: s, y packed [n], cu [B + 1], order (a permutation of the slates, or None), L = max_len"""

    def __init__(self, s, y, cu=None, order=None, L=None):
        self.s, self.y = np.ascontiguousarray(s, F), np.ascontiguousarray(y, F)
        self.cu = None if cu is None else np.asarray(cu, np.int32)
        self.order = None if order is None else np.asarray(order, np.int32)
        self.ragged = cu is not None
        self.B = len(cu) - 1 if self.ragged else self.s.shape[0]
        self.L = int(L if self.ragged else self.s.shape[1])

    def slates(self):
        """[(s_b, y_b, valid_b)] by slate index; n_b = len(s_b) is the extent the kernel's loops run to"""
        if not self.ragged:
            return [(self.s[b], self.y[b], self.y[b] != PAD) for b in range(self.B)]
        lo, hi = self.cu[:-1], np.minimum(self.cu[1:], self.cu[:-1] + self.L)
        return [(self.s[a:b], self.y[a:b], np.ones(max(b - a, 0), bool)) for a, b in zip(lo, hi)]

    def gather(self, rows, dtype=np.float64):
        """per-slate rows -> the layout of the gradient ([B, L] or packed)"""
        if not self.ragged:
            return np.stack([np.asarray(r, dtype) for r in rows])
        out = np.zeros(self.s.shape[0], dtype)
        for b, r in enumerate(rows):
            out[self.cu[b]:self.cu[b] + len(r)] = r
        return out


def _label_rank(y, valid):
    """stable descending counting rank among the valid items (ties: the lower index first); -1 for padded"""
    idx = np.flatnonzero(valid)
    rank = np.full(len(y), -1, np.int64)
    rank[idx[np.argsort(-f64(y)[idx], kind="stable")]] = np.arange(len(idx))
    return rank


def _gain(y):
    """(2^max(y, 0) - 1, its absolute error): exp2f P u 2^y, the subtraction u; a label 0 has gain 0 exactly"""
    p = np.exp2(np.maximum(f64(y), 0.0))
    g = p - 1.0
    return g, np.where(g == 0, 0.0, P_LIBM * U * p + U * g)


def _finalize(per, d_per, scale_abs):
    """out = scale * sum_b per[b] (ltrx_finalize_sum_kernel, 256 threads): k_block(ceil(B / 256), 256), the product 1, the scale's own
    rounding 1"""
    B = len(per)
    k = k_block(-(-B // 256), 256)
    tot, a = float(np.sum(per)), float(np.sum(np.abs(per)))
    e = float(np.sum(d_per))
    return tot, scale_abs * ((e + gam(k) * (a + e)) * (1 + gam(2)) + gam(2) * a)


# ---------------------------------------------------------------------------------------------------------------------------------
# ListNet
# ---------------------------------------------------------------------------------------------------------------------------------
def _softmax_err(x, valid, T):
    """(P, dP absolute) of expf(x - max) / sum over the valid items, in the kernel's chain"""
    n = len(x)
    P, dP = np.zeros(n), np.zeros(n)
    if not valid.any():
        return P, dP
    xm = np.where(valid, f64(x) - f64(x)[valid].max(), -np.inf)
    e = np.exp(xm)
    de = np.where(valid, np.expm1(U * np.abs(np.where(valid, xm, 0.0))) * (1 + P_LIBM * U) + P_LIBM * U, 0.0)
    ssum = e.sum()
    assert ssum >= 1.0
    k = k_block(-(-n // T), T)
    rel = comp(de, quot(de.max(), gam(k)), gam(2))
    P = e / ssum
    return P, np.where(valid, P * rel + 2 * FLT_MIN, 0.0)


def listnet_ref(bt, eps, batch_divisor):
    eps, inv = w(eps), 1.0 / w(batch_divisor)
    per, d_per, grads, bars = [], [], [], []
    for s, y, valid in bt.slates():
        n = len(s)
        P, dP = _softmax_err(s, valid, 256)
        T, dT = _softmax_err(y, valid, 256)
        assert (T[valid] > 2.0 ** -100).all(), "T > 0 is not clear of its threshold"
        k = k_block(-(-max(n, 1) // 256), 256)
        with np.errstate(divide="ignore", invalid="ignore"):
            lg = np.where(valid, np.log(P + eps), 0.0)
            rho = np.where(valid, (dP + U * (P + eps)) / (P + eps), 0.0)
            assert (rho < 0.5).all()
            dlog = -np.log1p(-rho) + P_LIBM * U * np.abs(lg)
            lt = T * lg
            dlt = dT * (np.abs(lg) + dlog) + T * dlog + U * (np.abs(lt) + T * dlog)
            r = np.where(valid, P / (P + eps), 0.0)
            dr = np.where(valid, ((P + dP) / (P + eps) / (1 - rho) * (1 + U) - r), 0.0)
        tr = T * r
        dtr = dT * (r + dr) + T * dr + U * (tr + dT * r + T * dr)
        rsum = tr.sum()
        d_rsum = dtr.sum() + gam(k) * (tr.sum() + dtr.sum())
        per.append(-lt.sum())
        d_per.append(dlt.sum() + gam(k) * (np.abs(lt).sum() + dlt.sum()))
        t1 = P * rsum
        dt1 = dP * (rsum + d_rsum) + P * d_rsum + U * (t1 + dP * rsum + P * d_rsum)
        S, E = t1 + tr, dt1 + dtr
        grads.append((t1 - tr) * inv)
        bars.append(np.where(valid, inv * ((E + U * (S + E)) * (1 + gam(2)) + gam(2) * S), 0.0))
    per, d_per = np.array(per), np.array(d_per)
    tot, d_loss = _finalize(per, d_per, inv)
    return dict(loss=tot * inv, per=per, grad=bt.gather(grads), bar_loss=d_loss, bar_per=d_per * (1 + U) + 0.0, bar_grad=bt.gather(bars),
                zero=bt.gather([~v for _, _, v in bt.slates()], bool))


def listnet_bar(ref):
    return dict(loss=ref["bar_loss"], per=ref["bar_per"], grad=ref["bar_grad"])


def _strided32(vals, T):
    """thread t adds vals[t], vals[t + T], ... serially: [T] partials"""
    n = len(vals)
    m = max(1, -(-n // T))
    pad = np.zeros(m * T, F)
    pad[:n] = vals
    acc = np.zeros(T, F)
    for k in range(m):
        acc = acc + pad[k * T:(k + 1) * T]
    return acc


def _block_sum32(per_thread):
    """block_sum: the wave tree, then the wave partials in order"""
    T = per_thread.size
    t = F(0)
    for v in _wave_sum(np.asarray(per_thread, F).reshape(T // 64, 64)):
        t = F(t + v)
    return t


def _scan32(a, T, exclusive=False, by_subtraction=False):
    """block_inclusive_scan of a copy of a"""
    a = np.asarray(a, F)
    n = len(a)
    chunk = -(-n // T)
    pad = np.zeros(chunk * T, F)
    pad[:n] = a
    pad = pad.reshape(T, chunk)
    for c in range(1, chunk):
        pad[:, c] = pad[:, c - 1] + pad[:, c]
    tot = pad[:, -1].copy()
    inc = tot.reshape(T // 64, 64).copy()
    o = 1
    while o < 64:
        nxt = inc.copy()
        nxt[:, o:] = inc[:, o:] + inc[:, :-o]
        inc, o = nxt, o * 2
    red = inc[:, 63].copy()
    base = inc - tot.reshape(T // 64, 64)                              # the defect model: rounded at the size of inc
    if not by_subtraction:
        base = np.concatenate([np.zeros((T // 64, 1), F), inc[:, :-1]], 1)
    for wv in range(T // 64):
        for k in range(wv):
            base[wv] = base[wv] + red[k]
    out = (pad + base.reshape(T, 1)).reshape(-1)[:n]
    if exclusive:
        out = (out - a).astype(F)
    return out.astype(F)


def _finalize32(per, scale):
    return F(F(scale) * _block_sum32(_strided32(np.asarray(per, F), 256)))


def _shifted(bt):
    """the defect `row0 = cu[b + 1]`: slate b reads its len items from the next slate's first row on (kept inside the packed rows)"""
    out = []
    for b in range(bt.B):
        n = int(min(bt.cu[b + 1] - bt.cu[b], bt.L))
        lo = int(min(bt.cu[b + 1], len(bt.s) - n))
        out.append((bt.s[lo:lo + n], bt.y[lo:lo + n], np.ones(n, bool)))
    return out


LISTNET_WRONG = ("r_one", "inv_div_twice", "per_slate_mean", "eps_dropped_in_r", "row0_off_by_one")


def listnet_f32(bt, eps, batch_divisor, wrong=None):
    eps, inv = F(eps), F(ONE / F(batch_divisor))
    per, grads = [], []
    sl = bt.slates()
    if wrong == "row0_off_by_one" and bt.ragged:
        sl = _shifted(bt)
    for s, y, valid in sl:
        n = len(s)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
            x = np.where(valid, s, -np.inf).astype(F)
            t = np.where(valid, y, -np.inf).astype(F)
            smax, ymax = (x.max(), t.max()) if n else (F(-np.inf), F(-np.inf))
            e = np.where(x == -np.inf, F(0), np.exp((x - smax).astype(F))).astype(F)
            f = np.where(t == -np.inf, F(0), np.exp((t - ymax).astype(F))).astype(F)
            ssum, ysum = _block_sum32(_strided32(e, 256)), _block_sum32(_strided32(f, 256))
            inv_s = ONE / ssum if ssum > 0 else F(0)
            inv_y = ONE / ysum if ysum > 0 else F(0)
            P, T = (e * inv_s).astype(F), (f * inv_y).astype(F)
            lt = np.where(T > 0, T * np.log(P + eps), F(0)).astype(F)
            rt = (T * (P / (P + eps))).astype(F)
            lsum, rsum = _block_sum32(_strided32(lt, 256)), _block_sum32(_strided32(rt, 256))
            if wrong == "r_one":
                r = np.where(P > 0, ONE, F(0)).astype(F)
            elif wrong == "eps_dropped_in_r":
                r = np.where(P > 0, P / P, F(0)).astype(F)
            else:
                r = np.where(P > 0, P / (P + eps), F(0)).astype(F)
            g = ((P * rsum - T * r) * inv).astype(F)
            if wrong == "inv_div_twice":
                g = (g * inv).astype(F)
            if wrong == "per_slate_mean":
                g = ((P * rsum - T * r) / F(max(int(valid.sum()), 1))).astype(F)
        per.append(F(-lsum))
        grads.append(g)
    return dict(loss=_finalize32(per, inv), per=np.array(per, F), grad=bt.gather(grads, F))


# ---------------------------------------------------------------------------------------------------------------------------------
# ListMLE (padded layout only)
# ---------------------------------------------------------------------------------------------------------------------------------
def _mle_order(y, perm):
    """original item index at sorted position r: the stable descending sort of the shuffled labels"""
    perm = np.asarray(perm, np.int64)
    return perm[np.argsort(-f64(y)[perm], kind="stable")]


def listmle_ref(bt, perm, eps, batch_divisor):
    eps, inv = w(eps), 1.0 / w(batch_divisor)
    L = bt.L
    T = block_threads("listmle", L)
    kb, ks = k_block(-(-L // T), T), k_scan(L, T)
    per, d_per, grads, bars, orders = [], [], [], [], []
    for s, y, _ in bt.slates():
        ord_ = _mle_order(y, perm)
        orders.append(ord_)
        ys, x = f64(y)[ord_], f64(s)[ord_]
        valid = ys != float(PAD)
        g, bar = np.zeros(L), np.zeros(L)
        if not valid.any():
            per.append(0.0), d_per.append(0.0), grads.append(g), bars.append(bar)
            continue
        xmax = x[valid].max()
        amax = int(np.flatnonzero(valid & (x == xmax))[0])
        xm = np.where(valid, x - xmax, 0.0)
        e = np.where(valid, np.exp(xm), 0.0)
        de = np.where(valid, np.expm1(U * np.abs(xm)) * (1 + P_LIBM * U) + P_LIBM * U, 0.0)
        ede = e * de + np.where(valid, FLT_MIN, 0.0)
        C = np.cumsum(e[::-1])[::-1]
        dC = np.cumsum(ede[::-1])[::-1]
        dC = dC + gam(ks) * (C + dC)
        rho = (dC + U * (C + eps)) / (C + eps)
        assert (rho[valid] < 0.5).all()
        lg = np.log(C + eps)
        dlog = -np.log1p(-rho) + P_LIBM * U * np.abs(lg)
        obs = np.where(valid, lg - xm, 0.0)
        dobs = np.where(valid, dlog + U * np.abs(xm) + U * (np.abs(obs) + dlog), 0.0)
        aobs = np.where(valid, np.abs(lg) + np.abs(xm), 0.0)
        per.append(obs.sum())
        d_per.append(dobs.sum() + gam(kb) * (aobs.sum() + dobs.sum()))
        q = np.where(valid, 1.0 / (C + eps), 0.0)
        dq = q * (quot(0.0, rho) * (1 + U) + U)
        Q = np.cumsum(q)
        dQ = np.cumsum(dq) + gam(ks) * (np.cumsum(q) + np.cumsum(dq))
        eq = e * Q
        gr = np.where(valid, eq - 1.0, 0.0)
        dg = np.where(valid, (e + ede) * (Q + dQ) * (1 + U) - eq + 2 * U * np.abs(gr), 0.0)
        gsum = gr.sum()
        d_gsum = dg.sum() + gam(kb) * (np.abs(gr).sum() + dg.sum())
        out = gr.copy()
        S, E = np.abs(gr), dg.copy()
        out[amax] -= gsum
        S[amax] += abs(gsum)
        E[amax] += d_gsum + U * (S[amax] + E[amax] + d_gsum)
        out, S, E = np.where(valid, out, 0.0), np.where(valid, S, 0.0), np.where(valid, E, 0.0)
        g[ord_] = out * inv
        bar[ord_] = inv * (E * (1 + gam(2)) + gam(2) * S)
        grads.append(g), bars.append(bar)
    per, d_per = np.array(per), np.array(d_per)
    tot, d_loss = _finalize(per, d_per, inv)
    return dict(loss=tot * inv, per=per, grad=np.stack(grads), order=np.stack(orders), bar_loss=d_loss, bar_per=d_per, bar_grad=np.stack(bars),
                zero=bt.y == PAD)


def listmle_bar(ref):
    return dict(loss=ref["bar_loss"], per=ref["bar_per"], grad=ref["bar_grad"])


LISTMLE_WRONG = ("no_argmax_correction", "eps_dropped_in_q", "exclusive_prefix", "exclusive_suffix", "tie_reversed", "inv_div_twice",
                 "argmax_last", "scan_base_by_subtraction")


def listmle_f32(bt, perm, eps, batch_divisor, wrong=None):
    eps, inv = F(eps), F(ONE / F(batch_divisor))
    L = bt.L
    T = block_threads("listmle", L)
    perm = np.asarray(perm, np.int64)
    per, grads, orders = [], [], []
    for s, y, _ in bt.slates():
        if wrong == "tie_reversed":                                   # pos[j] > pi: equal labels in reversed shuffled order
            ord_ = perm[::-1][np.argsort(-f64(y)[perm[::-1]], kind="stable")]
        else:
            ord_ = _mle_order(y, perm)
        orders.append(ord_)
        ys = y[ord_]
        with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
            xs = np.where(ys == PAD, -np.inf, s[ord_]).astype(F)
            xmax = xs.max()
            hit = np.flatnonzero(xs == xmax)
            amax = int(hit[-1] if wrong == "argmax_last" else hit[0]) if len(hit) else L
            ex = np.where(xs == -np.inf, F(0), np.exp((xs - xmax).astype(F))).astype(F)
            es = _scan32(ex[::-1], T, exclusive=wrong == "exclusive_suffix", by_subtraction=wrong == "scan_base_by_subtraction")
            C = es[::-1]
            valid = xs != -np.inf
            lt = np.where(valid, np.log(C + eps) - (xs - xmax), F(0)).astype(F)
            den = C if wrong == "eps_dropped_in_q" else (C + eps).astype(F)
            qs = np.where(valid, ONE / den, F(0)).astype(F)
            lsum = _block_sum32(_strided32(lt, T))
            Q = _scan32(qs, T, exclusive=wrong == "exclusive_prefix", by_subtraction=wrong == "scan_base_by_subtraction")
            g = np.where(valid, ex * Q - ONE, F(0)).astype(F)
            gsum = _block_sum32(_strided32(g, T))
            if wrong != "no_argmax_correction" and amax < L:
                g[amax] = g[amax] - gsum
            g = np.where(valid, g * inv, F(0)).astype(F)
            if wrong == "inv_div_twice":
                g = (g * inv).astype(F)
        out = np.zeros(L, F)
        out[ord_] = g
        per.append(lsum), grads.append(out)
    return dict(loss=_finalize32(per, inv), per=np.array(per, F), grad=np.stack(grads), order=np.stack(orders))


# ---------------------------------------------------------------------------------------------------------------------------------
# ApproxNDCG
# ---------------------------------------------------------------------------------------------------------------------------------
def _maxdcg(y, valid, rank, kk, disc, d_disc_rel, n, eps):
    """(maxDCG, its relative error): sum over the valid items with rank < kk of gain * disc[rank]; thread q = 0 walks i0, i0 + 256, .."""
    g, dg = _gain(y)
    use = valid & (rank < kk) & (rank >= 0)
    t = np.where(use, g * disc[np.maximum(rank, 0)], 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(t > 0, comp(np.where(g > 0, dg / np.where(g > 0, g, 1.0), 0.0), d_disc_rel, U), 0.0)
    dsum = t.sum()
    d_dsum = (t * rel).sum() + gam(k_block(-(-max(n, 1) // 256), 1024)) * (t * (1 + rel)).sum()
    assert dsum == 0 or dsum - 2 * d_dsum > eps, "maxDCG is not clear of its clamp"
    if dsum == 0:
        return eps, 0.0
    return dsum, d_dsum / dsum


def _expm1_up(x):
    """x + x^2 >= expm1(x) on 0 <= x < 1 (one pass over a pair matrix instead of a transcendental)"""
    return x + x * x


def _sg(z):
    """sigmoid(-z), sigmoid(z) and the relative error of the former as sigmoid_neg_fast computes it"""
    e = np.exp(np.clip(z, -700.0, 700.0))
    sg = 1.0 / (1.0 + e)
    sgc = e * sg
    return sg, sgc, comp((_expm1_up(gam(4) * np.abs(z)) * (1 + P_HW * U) + P_HW * U) * sgc, U, P_HW * U)


def approxndcg_ref(bt, eps, alpha, batch_divisor, strict=True):
    eps, alpha, inv = w(eps), w(alpha), 1.0 / w(batch_divisor)
    per, d_per, grads, bars, bad = [], [], [], [], []
    for b, (s, y, valid) in enumerate(bt.slates()):
        n = len(s)
        g, bar = np.zeros(n), np.zeros(n)
        idx = np.flatnonzero(valid)
        if not len(idx):
            per.append(0.0), d_per.append(0.0), grads.append(g), bars.append(bar)
            continue
        rank = _label_rank(y, valid)
        disc = 1.0 / np.log2(2.0 + np.arange(n))
        M, dM = _maxdcg(y, valid, rank, n + 1, disc, comp(P_LIBM * U, 0.0), n, eps)
        gain, dgain = _gain(y[idx])
        G = gain / M
        dG = np.where(gain > 0, G * comp(np.where(gain > 0, dgain / np.where(gain > 0, gain, 1.0), 0.0), quot(0.0, dM), U), 0.0)
        sv = f64(s)[idx]
        nv = len(idx)
        kp = k_pair(n)
        pos, dpos = np.zeros(nv), np.zeros(nv)
        for lo in range(0, nv, CHUNK):
            I = slice(lo, min(nv, lo + CHUNK))
            z = alpha * (sv[I, None] - sv[None, :])
            sg, sgc, dsg = _sg(z)
            c = np.maximum(sg, eps)
            err = np.where(sg >= eps, sg * dsg, 0.0)
            band = np.abs(sg - eps) <= 2 * sg * dsg
            r = np.arange(I.start, I.stop)
            c[r - lo, r], err[r - lo, r], band[r - lo, r] = 0.0, 0.0, False
            if band.any():
                bad.extend((b, int(idx[lo + i])) for i in np.unique(np.nonzero(band)[0]))
            pos[I] = c.sum(1)
            dpos[I] = err.sum(1)
        dpos = dpos + gam(kp + 1) * (1.0 + pos + dpos)
        pos = 1.0 + pos
        rho = dpos / (1.0 + pos) + U
        aD = np.log2(1.0 + pos)
        daD = rho / (LN2 * (1 - rho)) / aD + P_LIBM * U                       # relative
        v = G / aD
        dv = np.where(G > 0, v * comp(np.where(G > 0, dG / np.where(G > 0, G, 1.0), 0.0), quot(0.0, daD), U), 0.0)
        kb = k_block(-(-n // 256), 1024)
        per.append(v.sum())
        d_per.append(dv.sum() + gam(kb) * (v.sum() + dv.sum()))
        wt = G / (aD * aD * (1.0 + pos) * LN2)
        dw = np.where(G > 0, wt * comp(np.where(G > 0, dG / np.where(G > 0, G, 1.0), 0.0), quot(0.0, 2 * daD + rho + gam(4)), U), 0.0)
        acc, A, E = np.zeros(nv), np.zeros(nv), np.zeros(nv)
        for lo in range(0, nv, CHUNK):
            I = slice(lo, min(nv, lo + CHUNK))
            z = alpha * (sv[I, None] - sv[None, :])
            sg, sgc, dsg = _sg(z)
            ds = sg * sgc
            e1 = sg * dsg + FLT_MIN                                     # a sigmoid below FLT_MIN is flushed or denormal
            e2 = e1 + U * (sgc + e1)
            d_ds = (sg + e1) * (sgc + e2) * (1 + U) - ds
            on_a, on_c = sgc >= eps, sg >= eps
            a, da = np.where(on_a, wt[None, :], 0.0), np.where(on_a, dw[None, :], 0.0)
            c, dc = np.where(on_c, wt[I, None], 0.0), np.where(on_c, dw[I, None], 0.0)
            term = ds * (a - c)
            terr = (d_ds * (wt[None, :] + wt[I, None]) + np.where(on_a, 0.0, ds * wt[None, :]) + (ds + d_ds) * (da + dc)
                    + 2 * U * (ds + d_ds) * (a + c + da + dc) + FLT_MIN)
            tabs = ds * (a + c)
            r = np.arange(I.start, I.stop)
            term[r - lo, r], terr[r - lo, r], tabs[r - lo, r] = 0.0, 0.0, 0.0
            acc[I], A[I], E[I] = term.sum(1), tabs.sum(1), terr.sum(1)
        g[idx] = alpha * acc * inv
        bar[idx] = alpha * inv * (E + gam(kp + 3) * (A + E))
        grads.append(g), bars.append(bar)
    if strict:
        assert not bad, "approxNDCG: sg is inside the band around eps for items %s" % bad[:8]
    per, d_per = np.array(per), np.array(d_per)
    tot, d_loss = _finalize(per, d_per, inv)
    return dict(loss=-tot * inv, per=per, grad=bt.gather(grads), bar_loss=d_loss, bar_per=d_per, bar_grad=bt.gather(bars), violations=bad,
                zero=bt.gather([~v for _, _, v in bt.slates()], bool))


def approxndcg_bar(ref):
    return dict(loss=ref["bar_loss"], per=ref["bar_per"], grad=ref["bar_grad"])


DROP = {"quarter_tail_dropped": "last", "lq_rounded_down": "floor"}


def _quarters(n, drop_tail=False):
    """drop_tail "last": every quarter walks one partner short; "floor": lq = n >> 2, so the n % 4 last items are nobody's partner"""
    lq = (n >> 2) if drop_tail == "floor" else (n + 3) >> 2
    out = []
    for q in range(4):
        j0 = q * lq
        j1 = min(n, j0 + lq)
        if drop_tail == "last" and j1 > j0:
            j1 = min(n, j0 + lq - 1) if j0 + lq <= n else j1 - 1
        out.append((j0, max(j0, j1)))
    return out


def _quarter_sum32(mats, n, drop_tail=False):
    """[(sign, M [rows, n])]: per row and quarter the serial walk over the partners, every matrix in turn per partner; then (p0 + p1) +
    (p2 + p3).  A skipped partner is a 0.f term (adding 0.f is exact)."""
    rows = mats[0][1].shape[0]
    parts = []
    for j0, j1 in _quarters(n, drop_tail):
        acc = np.zeros(rows, F)
        for j in range(j0, j1):
            for sign, M in mats:
                acc = acc + M[:, j] if sign > 0 else acc - M[:, j]
        parts.append(acc)
    return ((parts[0] + parts[1]) + (parts[2] + parts[3])).astype(F)


def _q0_block_sum32(vals, n):
    """the threads of quarter 0 own items i0, i0 + 256, ..; the other 768 threads add 0.f; block_sum over 1024 threads"""
    per = np.zeros(1024, F)
    per[:256] = _strided32(vals, 256)
    return _block_sum32(per)


def _count_rank32(key, n, skip, drop_tail=False, reverse_tie=False, count_padded=False):
    """the counting rank of every item over the quarters (an integer sum: exact)"""
    key = f64(key)
    j = np.arange(n)
    first = (j[None, :] > j[:, None]) if reverse_tie else (j[None, :] < j[:, None])
    before = (key[None, :] > key[:, None]) | ((key[None, :] == key[:, None]) & first)
    if not count_padded:
        before = before & ~skip[None, :]
    rank = np.zeros(n, np.int64)
    for j0, j1 in _quarters(n, drop_tail):
        rank += before[:, j0:j1].sum(1)
    return rank


# Not in the list because they are the same function, not defects -- so of the two clamps of pass 2 only `sg >= eps` has a defect model
# ("each clamp" cannot be shown for `1 - sg >= eps`: leaving it out changes no bit): the label rank feeds maxDCG alone, a sum over the multiset of (gain,
# rank) that a tie broken the other way leaves unchanged, and a padded label (-1) is below every valid one, so it is never counted
# whether skipped or not; `1 - sg >= eps` is false in fp32 only where 1 - sg == 0, and then ds == 0 whatever a is.  (All three are
# kept as switches of approxndcg_f32; tests/test_listwise_ref_cpu.py asserts that they change no bit -- the tie-break, which hands the
# same ranks to other threads, no more than the order of maxDCG's sum.)
APPROX_SAME = ("tie_reversed", "padded_counted", "clamp_a_not_zeroed")
APPROX_WRONG = ("quarter_tail_dropped", "lq_rounded_down", "discount_at_rank", "clamp_c_not_zeroed",
                "w_without_pos_factor", "a_c_swapped", "inv_div_twice", "row0_off_by_one", "alpha_dropped_in_grad")


def approxndcg_f32(bt, eps, alpha, batch_divisor, wrong=None):
    eps, alpha, inv = F(eps), F(alpha), F(ONE / F(batch_divisor))
    drop = DROP.get(wrong, False)
    per, grads = [], []
    sl = bt.slates()
    if wrong == "row0_off_by_one" and bt.ragged:
        sl = _shifted(bt)
    for s, y, valid in sl:
        n = len(s)
        if n == 0:
            per.append(F(0)), grads.append(np.zeros(0, F))
            continue
        pad = ~valid
        with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
            rank = _count_rank32(y, n, pad, drop, wrong == "tie_reversed", wrong == "padded_counted").astype(F)
            gain = (np.exp2(np.maximum(y, F(0))).astype(F) - ONE).astype(F)
            first_pos = ONE if wrong == "discount_at_rank" else F(2)
            dterm = np.where(valid, gain / np.log2((first_pos + rank).astype(F)).astype(F), F(0)).astype(F)
            if wrong == "discount_at_rank":
                dterm = np.where(np.isfinite(dterm), dterm, F(0)).astype(F)
            maxdcg = np.maximum(_q0_block_sum32(dterm, n), eps)
            z = ((alpha * (s[:, None] - s[None, :]).astype(F)).astype(F) * F(LOG2E)).astype(F)
            sg = (ONE / (ONE + np.exp2(z).astype(F)).astype(F)).astype(F)
            live = valid[:, None] & valid[None, :] & ~np.eye(n, dtype=bool)
            c = np.where(live, np.maximum(sg, eps), F(0)).astype(F)
            pos = (ONE + _quarter_sum32([(1, c)], n, drop)).astype(F)
            G = (gain / maxdcg).astype(F)
            aD = np.log2((ONE + pos).astype(F)).astype(F)
            v = np.where(valid, G / aD, F(0)).astype(F)
            if wrong == "w_without_pos_factor":
                wt = np.where(valid, G / (aD * aD), F(0)).astype(F)
            else:
                wt = np.where(valid, G / (((aD * aD).astype(F) * (ONE + pos)).astype(F) * F(0.6931471805599453)).astype(F), F(0)).astype(F)
            vsum = _q0_block_sum32(v, n)
            one_m = (ONE - sg).astype(F)
            ds = (sg * one_m).astype(F)
            a = np.where((one_m >= eps) | (wrong == "clamp_a_not_zeroed"), wt[None, :], F(0)).astype(F)
            cc = np.where((sg >= eps) | (wrong == "clamp_c_not_zeroed"), wt[:, None], F(0)).astype(F)
            diff = (cc - a) if wrong == "a_c_swapped" else (a - cc)
            term = np.where(live, ds * diff.astype(F), F(0)).astype(F)
            acc = _quarter_sum32([(1, term)], n, drop)
            g = np.where(valid, ((acc if wrong == "alpha_dropped_in_grad" else alpha * acc).astype(F) * inv).astype(F), F(0)).astype(F)
            if wrong == "inv_div_twice":
                g = (g * inv).astype(F)
        per.append(vsum), grads.append(g)
    return dict(loss=_finalize32(per, -inv), per=np.array(per, F), grad=bt.gather(grads, F))


# ---------------------------------------------------------------------------------------------------------------------------------
# LambdaLoss
# ---------------------------------------------------------------------------------------------------------------------------------
Lam = namedtuple("Lam", "scheme k sigma mu mean natural ext")          # k <= 0: none; ext: ext_pair_count (None: NULL)
D_INVD = comp(P_LIBM * U, U)


def _weights(scheme, mu, Ga, dGa, ra, ya, Gb, dGb, rb, yb, invD):
    """(w, dw absolute) of the ordered pairs (a = rows [:, None], b = columns [None, :]) in fp64"""
    if scheme in (0, 5):
        return np.ones((len(Ga), len(Gb))), 0.0
    A, B = (slice(None), None), (None, slice(None))
    if scheme == 1:
        wv = Ga * invD[ra + 1]
        dwv = (Ga + dGa) * invD[ra + 1] * (1 + D_INVD) * (1 + U) - wv
        return np.broadcast_to(wv[A], (len(Ga), len(Gb))), np.broadcast_to(dwv[A], (len(Ga), len(Gb)))
    if scheme in (6, 7):
        if scheme == 6:
            wv = np.abs(ya[A] - yb[B])
            return wv, U * wv
        wv = np.abs(ya[A] ** 2 - yb[B] ** 2)
        return wv, U * (ya[A] ** 2 + yb[B] ** 2) + U * wv
    dg = np.abs(Ga[A] - Gb[B])
    ddg = dGa[A] + dGb[B] + U * dg
    out_w, out_d = 0.0, 0.0
    if scheme in (2, 4):
        d = np.abs(ra[A] - rb[B])
        hi, lo = invD[d], invD[d + 1]
        dl = np.where(d == 0, 0.0, np.abs(hi - lo))
        ddl = np.where(d == 0, 0.0, D_INVD * (hi + lo) + U * dl)
        t = dl * dg
        dt = (dl + ddl) * (dg + ddg) * (1 + U) - t
        if scheme == 2:
            return t, dt
        out_w, out_d = mu * t, mu * (dt + U * (t + dt))
    hi, lo = invD[ra + 1][A], invD[rb + 1][B]
    lr = np.abs(hi - lo)
    dlr = D_INVD * (hi + lo) + U * lr
    t = lr * dg
    dt = (lr + dlr) * (dg + ddg) * (1 + U) - t
    wv = out_w + t
    return wv, out_d + dt + U * (wv + out_d + dt)


def lambdaloss_ref(bt, eps, p, strict=True):
    eps, sigma, mu = w(eps), w(p.sigma), w(p.mu)
    ln_eps, ilnb = float(np.log(eps)), (1.0 if p.natural else LOG2E)
    d_lneps = P_LIBM * U * abs(ln_eps)
    allp = p.scheme == ALL_PAIRS
    per, d_per, cnt, grads, bars, aabs, orders, bad = [], [], [], [], [], [], [], []
    for b, (s, y, valid) in enumerate(bt.slates()):
        n = len(s)
        g, bar, ab = np.zeros(n), np.zeros(n), np.zeros(n)
        nvalid = int(valid.sum())
        rs = _label_rank(s, valid)
        order = np.concatenate([np.flatnonzero(valid)[np.argsort(rs[valid], kind="stable")], np.flatnonzero(~valid)]).astype(np.int64)
        orders.append(order)
        if nvalid == 0:
            per.append(0.0), d_per.append(0.0), cnt.append(0.0), grads.append(g), bars.append(bar), aabs.append(ab)
            continue
        kk = n if (p.k <= 0 or p.k > n) else p.k
        ry = _label_rank(y, valid)
        invD = np.concatenate([[0.0], 1.0 / np.log2(1.0 + np.arange(1, n + 2))])
        M, dM = _maxdcg(y, valid, ry, kk, invD[1:], D_INVD, n, eps)
        act = np.flatnonzero(valid & (rs < kk))
        ya = np.maximum(f64(y)[act], 0.0)
        gain, dgain = _gain(y[act])
        G = gain / M
        dG = np.where(gain > 0, G * comp(np.where(gain > 0, dgain / np.where(gain > 0, gain, 1.0), 0.0), quot(0.0, dM), U), 0.0)
        sa, ra, yraw = f64(s)[act], rs[act], f64(y)[act]
        na = len(act)
        row, col, rowE, colE = (np.zeros(na) for _ in range(4))
        lsum = labs = lerr = 0.0
        count = 0
        for lo in range(0, na, CHUNK):
            I = slice(lo, min(na, lo + CHUNK))
            sel = np.ones((I.stop - lo, na), bool) if allp else (yraw[I, None] > yraw[None, :])
            dx = sigma * (sa[I, None] - sa[None, :])
            e = np.exp(np.clip(dx, -700.0, 700.0))
            sigc = 1.0 / (1.0 + e)
            sig = e * sigc
            dE = _expm1_up(gam(2) * np.abs(dx)) * (1 + P_LIBM * U) + P_LIBM * U
            dsig = comp(dE * sigc, U, U)
            W, dW = _weights(p.scheme, mu, G[I], dG[I], ra[I], ya[I], G, dG, ra, ya, invD)
            on = sig >= eps
            band = sel & (np.abs(sig - eps) <= 2 * sig * dsig)
            lq_ = np.log(np.maximum(sig, eps))
            dlog = np.where(on, dsig / (1 - dsig), 0.0) + P_LIBM * U * np.abs(lq_)
            wl = W * lq_
            d_wl = dW * np.abs(lq_) + (W + dW) * dlog + U * np.abs(wl)
            band |= sel & on & (np.abs(wl - ln_eps) <= 2 * (d_wl + d_lneps))
            if band.any():
                bad.extend((b, int(act[lo + i])) for i in np.unique(np.nonzero(band)[0]))
            l = np.where(sel, np.maximum(wl, ln_eps) * ilnb, 0.0)
            le = np.where(sel, np.maximum(d_wl, d_lneps) * ilnb * (1 + gam(2)) + gam(2) * np.abs(l), 0.0)
            lsum, labs, lerr = lsum + l.sum(), labs + np.abs(l).sum(), lerr + le.sum()
            count += int(sel.sum())
            live = sel & on & (wl >= ln_eps)
            r = np.arange(I.start, I.stop)
            live[r - lo, r] = False
            gm = np.where(live, W * sigma * sigc * ilnb, 0.0)
            ge = np.where(live, (dW * sigma * sigc + (W + dW) * sigma * (sig * dsig + U * sigc)) * ilnb * (1 + gam(4)) + gam(4) * gm, 0.0)
            row[I], rowE[I] = gm.sum(1), ge.sum(1)
            col, colE = col + gm.sum(0), colE + ge.sum(0)
        kp = k_pair(n, allp)
        g[act] = -row + col
        ab[act] = row + col
        bar[act] = (rowE + colE) + gam(kp) * (row + col + rowE + colE)
        m = -(-n // 256) * ((n + 3) >> 2) * (2 if allp else 1)
        per.append(lsum), d_per.append(lerr + gam(k_block(m, 1024)) * (labs + lerr)), cnt.append(float(count))
        grads.append(g), bars.append(bar), aabs.append(ab)
    if strict:
        assert not bad, "lambdaLoss: a clamp decision is inside its band for items %s" % bad[:8]
    per, d_per = np.array(per), np.array(d_per)
    total = float(np.sum(cnt))
    assert total < 2 ** 24, "the pair count is no longer an exact fp32 sum"
    div = 1.0 if not p.mean else (w(p.ext) if p.ext is not None else total)
    a, d_a = _finalize(per, d_per, 1.0)
    grad, bg, ag = bt.gather(grads), bt.gather(bars), bt.gather(aabs)
    with np.errstate(divide="ignore", invalid="ignore"):
        loss = -a / div if div != 0 else np.nan
        bar_loss = (d_a * (1 + U) + U * abs(a)) / div if div > 0 else 0.0
        if p.mean:
            sc = 1.0 / div if div > 0 else 0.0
            grad, bg = grad * sc, (bg * (1 + gam(2)) + gam(2) * ag) * sc
    return dict(loss=loss, per=per, count=total, grad=grad, order=bt.gather(orders, np.int64), bar_loss=bar_loss, bar_per=d_per, bar_grad=bg,
                violations=bad, zero=bt.gather([~v for _, _, v in bt.slates()], bool))


def lambdaloss_bar(ref):
    return dict(loss=ref["bar_loss"], per=ref["bar_per"], grad=ref["bar_grad"])


LAMBDA_WRONG = ("quarter_tail_dropped", "lq_rounded_down", "tie_reversed", "padded_counted", "discount_at_rank", "rj_gt_kk", "diag_grad_kept", "bwd_from_one_minus",
                "clamp_sig_not_zeroed", "clamp_wl_not_zeroed", "mean_per_slate", "mu_dropped", "maxdcg_all_ranks", "row0_off_by_one")


def _weights32(scheme, mu, Ga, ra, ya, Gb, rb, yb, invD):
    A, B = (slice(None), None), (None, slice(None))
    shape = (len(Ga), len(Gb))
    if scheme in (0, 5):
        return np.ones(shape, F)
    if scheme == 1:
        return np.broadcast_to((Ga * invD[ra + 1]).astype(F)[A], shape)
    if scheme == 6:
        return np.abs(ya[A] - yb[B]).astype(F)
    if scheme == 7:
        return np.abs((ya * ya).astype(F)[A] - (yb * yb).astype(F)[B]).astype(F)
    dg = np.abs(Ga[A] - Gb[B]).astype(F)
    lr = (np.abs(invD[ra + 1][A] - invD[rb + 1][B]).astype(F) * dg).astype(F)
    if scheme == 3:
        return lr
    d = np.abs(ra[A] - rb[B])
    dl = np.where(d == 0, F(0), np.abs(invD[d] - invD[d + 1])).astype(F)
    if scheme == 2:
        return (dl * dg).astype(F)
    return ((F(mu) * (dl * dg).astype(F)).astype(F) + lr).astype(F)


def _pair_terms32(W, sig, eps, ln_eps, sigma, ilnb, wrong):
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        q = np.maximum(sig, eps)
        wl = (W * np.log(q).astype(F)).astype(F)
        live = ((sig >= eps) | (wrong == "clamp_sig_not_zeroed")) & ((wl >= ln_eps) | (wrong == "clamp_wl_not_zeroed"))
        l = (np.maximum(wl, ln_eps) * ilnb).astype(F)
        g = np.where(live, (((W * sigma).astype(F) * (ONE - sig).astype(F)).astype(F) * ilnb).astype(F), F(0)).astype(F)
    return l, g


def lambdaloss_f32(bt, eps, p, wrong=None):
    eps, sigma, mu = F(eps), F(p.sigma), F(0.0 if wrong == "mu_dropped" else p.mu)
    ln_eps = np.log(eps).astype(F)
    ilnb = ONE if p.natural else F(LOG2E)
    allp = p.scheme == ALL_PAIRS
    drop = DROP.get(wrong, False)
    per, cnt, grads, orders = [], [], [], []
    sl = bt.slates()
    if wrong == "row0_off_by_one" and bt.ragged:
        sl = _shifted(bt)
    for s, y, valid in sl:
        n = len(s)
        if n == 0:
            per.append(F(0)), cnt.append(F(0)), grads.append(np.zeros(0, F)), orders.append(np.zeros(0, np.int64))
            continue
        pad = ~valid
        kk = n if (p.k <= 0 or p.k > n) else p.k
        with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
            invD = np.concatenate([[F(0)], (ONE / np.log2((ONE + np.arange(1, n + 2).astype(F)).astype(F)).astype(F)).astype(F)]).astype(F)
            rs = _count_rank32(s, n, pad, drop, wrong == "tie_reversed", wrong == "padded_counted")
            ry = _count_rank32(y, n, pad, drop, wrong == "tie_reversed", wrong == "padded_counted")
            rk = np.where(valid, rs, bt.L)
            gain = (np.exp2(np.maximum(y, F(0))).astype(F) - ONE).astype(F)
            use = valid & ((ry < kk) | (wrong == "maxdcg_all_ranks"))
            dterm = np.where(use, gain * invD[np.minimum(ry + (0 if wrong == "discount_at_rank" else 1), n + 1)], F(0)).astype(F)
            maxdcg = np.maximum(_q0_block_sum32(dterm, n), eps)
            G = np.where(valid, gain / maxdcg, F(0)).astype(F)
            order = np.zeros(n, np.int64)
            nv = int(valid.sum())
            vi = np.flatnonzero(valid)
            if len(set(rk[vi].tolist())) == nv and (rk[vi] < nv).all():
                order[rk[vi]] = vi
            order[nv:] = np.flatnonzero(pad)
            yc = np.maximum(y, F(0))
            rr = np.minimum(rk, n)
            in_k = valid & ((rk <= kk) if wrong == "rj_gt_kk" else (rk < kk))
            rowk = valid & (rk < kk)
            both = rowk[:, None] & in_k[None, :]
            eye = np.eye(n, dtype=bool)
            fwd = both & (True if allp else (y[:, None] > y[None, :]))
            bwd = both & ~eye & (True if allp else (y[None, :] > y[:, None]))
            dx = (sigma * (s[:, None] - s[None, :]).astype(F)).astype(F)
            sig_f = (ONE / (ONE + np.exp(-dx).astype(F)).astype(F)).astype(F)
            sig_b = (ONE - sig_f).astype(F) if wrong == "bwd_from_one_minus" else (ONE / (ONE + np.exp(dx).astype(F)).astype(F)).astype(F)
            Wf = _weights32(p.scheme, mu, G, rr, yc, G, rr, yc, invD)
            Wb = Wf.T                                                     # pair (j, i): first = j
            lf, gf = _pair_terms32(Wf, sig_f, eps, ln_eps, sigma, ilnb, wrong)
            _, gb = _pair_terms32(Wb, sig_b, eps, ln_eps, sigma, ilnb, wrong)
            lf = np.where(fwd, lf, F(0)).astype(F)
            gf = np.where(fwd & (~eye | (wrong == "diag_grad_kept")), gf, F(0)).astype(F)
            gb = np.where(bwd, gb, F(0)).astype(F)
            g = _quarter_sum32([(-1, gf), (1, gb)], n, drop)
            lthr, cthr = np.zeros(1024, F), np.zeros(1024, F)
            for q, (j0, j1) in enumerate(_quarters(n, drop)):
                for m in range(0, n, 256):
                    rws = slice(m, min(n, m + 256))
                    k = rws.stop - m
                    for j in range(j0, j1):
                        lthr[q * 256:q * 256 + k] = lthr[q * 256:q * 256 + k] + lf[rws, j]
                    cthr[q * 256:q * 256 + k] = cthr[q * 256:q * 256 + k] + fwd[rws, j0:j1].sum(1).astype(F)
            per.append(_block_sum32(lthr)), cnt.append(_block_sum32(cthr)), grads.append(g), orders.append(order)
    a = _block_sum32(_strided32(np.array(per, F), 256))
    c = _block_sum32(_strided32(np.array(cnt, F), 256))
    div = (F(p.ext) if p.ext is not None else c) if p.mean else ONE
    with np.errstate(divide="ignore", invalid="ignore"):
        loss = F(-a / div)
        sc = ONE / div if div > 0 else F(0)
    if p.mean:
        if wrong == "mean_per_slate":
            grads = [(gq * (ONE / cq if cq > 0 else F(0))).astype(F) for gq, cq in zip(grads, cnt)]
        else:
            grads = [(gq * sc).astype(F) for gq in grads]
    return dict(loss=loss, per=np.array(per, F), count=float(c), grad=bt.gather(grads, F), order=bt.gather(orders, np.int64))


# ---------------------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------------------
# lambdaLoss: the whole matrix 8 schemes x (k none, 5, L, L + 3) x (sum binary, mean natural) at every L <= 257 and both score scales (+
# ext_pair_count, + the cut at L - 1 from L = 255); beyond 257 two schemes (lambdaRank, ndcgLoss2PP k 5 mean): the fp64 pair passes are
# O(L^2), and the schemes differ in the weight of a pair, not in the walk a long slate changes.  "low tail" cases: see _draw.
# arm: "LDS", "LDS opt-in" (more than the default dynamic allowance) or "GWS".  listNet has no reachable GWS arm: at
# LTRX_MAX_LONG_SLATE_LEN its two arrays are 128 KB, inside the budget; its table ends at the opt-in threshold.
Case = namedtuple("Case", "name loss layout L scale arm par order long low_tail")
LOW_TAIL_GAP = 6.0
EPS = 1e-10
SHORT = (1, 2, 3, 4, 5, 255, 256, 257)
KILO = (1023, 1024, 1025)
RAGGED_LENGTHS = (0, 1, 2, 3, 5, 31, 32, 33, 64, 100, 255, 256, 257)     # tests/ragged_cases.py's batch
MAX_F32_L = 1025


# the arm every threshold length must take, as literals (the table's own `arm` comes from the restated rule)
EXPECTED_ARMS = {("lambdaloss", 945): "LDS", ("lambdaloss", 946): "LDS opt-in", ("lambdaloss", 3130): "LDS opt-in", ("lambdaloss", 3131): "GWS",
                 ("approxndcg", 1755): "LDS", ("approxndcg", 1756): "LDS opt-in", ("approxndcg", 5814): "LDS opt-in", ("approxndcg", 5815): "GWS",
                 ("listmle", 2048): "LDS", ("listmle", 2049): "LDS opt-in", ("listmle", 6784): "LDS opt-in", ("listmle", 6785): "GWS",
                 ("listnet", 6144): "LDS", ("listnet", 6145): "LDS opt-in", ("listnet", 257): "LDS", ("lambdaloss", 1025): "LDS opt-in"}


def arm_of(loss, L):
    return "GWS" if not in_lds(loss, L) else ("LDS opt-in" if opts_in(loss, L) else "LDS")


def thresholds(loss):
    a, b = last_lds(loss, DEFAULT_DYN_LDS), last_lds(loss)
    return (a, a + 1) + ((b, b + 1) if b < MAX_LONG else ())


def _lam_configs(L):
    ks = sorted({0, 5, L, L + 3})                            # none, 5, L, above L (L = 5: three of them)
    return [Lam(sc, k, 1.3, 7.0, mean, mean, None) for sc in range(8) for k in ks for mean in (False, True)]


def _cases():
    out = []

    def add(loss, layout, L, scale, par, tag, order=False, low_tail=False):
        long = L > MAX_F32_L
        name = "%s %s L %d x%d %s%s" % (loss, layout, L, scale, tag, " low tail" if low_tail else "")
        out.append(Case(name, loss, layout, L, scale, arm_of(loss, L), par, order, long, low_tail))

    for loss in ("listnet", "listmle", "approxndcg", "lambdaloss"):
        lengths = SHORT + ((512, 513) if loss == "listmle" else ()) + (KILO if loss != "listnet" else (1024,)) + thresholds(loss)
        for L in lengths:
            for scale in ((1, 30) if L <= 257 or (loss, L) == ("listmle", 512) else (1,)):      # 512: two items per thread of the scan
                if loss == "listnet":
                    add(loss, "padded", L, scale, None, "")
                elif loss == "listmle":
                    add(loss, "padded", L, scale, "identity", "identity")
                    add(loss, "padded", L, scale, "seeded", "seeded perm")
                elif loss == "approxndcg":
                    for alpha in (1.0, 2.5):
                        add(loss, "padded", L, scale, alpha, "alpha %g" % alpha)
                else:
                    cfg = _lam_configs(L)
                    if L > 257:                               # the long lengths: two schemes, as the pair passes are O(L^2) in fp64
                        pick = [Lam(3, 0, 1.3, 7.0, False, False, None), Lam(4, 5, 1.3, 7.0, True, True, None)]
                    else:                                     # the whole matrix at every short length and both score scales
                        pick = cfg + [Lam(3, 5, 1.3, 7.0, True, True, 17.0)]          # + ext_pair_count given
                        if L >= 255:                          # the cut one above the last rank: at scale 30 the item it excludes is far below
                            pick += [Lam(3, L - 1, 1.3, 7.0, False, False, None), Lam(0, L - 1, 1.3, 7.0, True, True, None)]
                    for p in pick:
                        add(loss, "padded", L, scale, p, "%s k %d %s%s" % (SCHEMES[p.scheme], p.k, "mean natural" if p.mean else "sum binary",
                                                                           "" if p.ext is None else " ext count"))
    # the last item far below the rest with label 0: partners beyond four whole quarters are near saturation and move no rank
    for L in (5, 257):
        for p in (Lam(0, 0, 1.3, 7.0, False, False, None), Lam(3, 0, 1.3, 7.0, False, False, None), Lam(5, 0, 1.3, 7.0, True, True, None),
                  Lam(6, 0, 1.3, 7.0, False, False, None)):
            add("lambdaloss", "padded", L, 1, p, "%s k %d %s" % (SCHEMES[p.scheme], p.k, "mean natural" if p.mean else "sum binary"), low_tail=True)
        add("approxndcg", "padded", L, 1, 1.0, "alpha 1", low_tail=True)
    for order in (False, True):
        tag = "slate_order" if order else "in order"
        for scale in (1, 30):
            add("listnet", "ragged", 257, scale, None, tag, order)
            add("approxndcg", "ragged", 257, scale, 1.0, "alpha 1 " + tag, order)
            add("approxndcg", "ragged", 257, scale, 2.5, "alpha 2.5 " + tag, order)
            for p in (Lam(1, 0, 1.3, 7.0, False, False, None), Lam(3, 0, 1.3, 7.0, True, True, None), Lam(4, 5, 1.3, 7.0, True, True, None),
                      Lam(2, 5, 1.3, 7.0, False, False, None), Lam(7, 0, 1.3, 7.0, True, True, 17.0)):
                add("lambdaloss", "ragged", 257, scale, p, "%s k %d %s %s" % (SCHEMES[p.scheme], p.k, "mean" if p.mean else "sum", tag), order)
    add("approxndcg", "ragged", last_lds("approxndcg") + 1, 1, 1.0, "alpha 1 long", True)
    add("lambdaloss", "ragged", last_lds("lambdaloss") + 1, 1, Lam(4, 5, 1.3, 7.0, True, True, None), "ndcgLoss2PP k 5 mean long", True)
    add("lambdaloss", "ragged", last_lds("lambdaloss") + 1, 1, Lam(3, 0, 1.3, 7.0, False, False, None), "lambdaRank sum long", False)
    return out


CASES = _cases()


def valid_counts(c):
    """the number of leading valid items per slate of a padded case"""
    L = c.L
    if c.arm == "GWS" or c.long:
        return (L, L // 2 + 1, 37)                             # B = 3: blockIdx.x * gws_stride matters, different valid counts
    return (L, max(1, L - 1), 0, -(-L // 2))                   # full; all labels 0 with one padded slot; fully padded; half


def _draw(c):
    seed = [sum(map(ord, c.loss)), c.L, c.scale, int(c.layout == "ragged")]
    rng = np.random.default_rng(seed)
    if c.layout == "ragged":
        lengths = RAGGED_LENGTHS if c.L == 257 else (5, 0, c.L, 1, 100)
        ss, ys = [], []
        for b, n in enumerate(lengths):
            s, y = rng.standard_normal(n), rng.integers(0, 5, n).astype(np.float64)
            if b in (7, 10) and c.L == 257:
                s = np.round(s * 4) / 4
            elif n >= 2:
                s[-1] = s[0]
            if b == 5 and c.L == 257:
                y[:] = 0
            ss.append(s), ys.append(y)
        cu = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
        order = rng.permutation(len(lengths)).astype(np.int32) if c.order else None
        s = (np.concatenate(ss).astype(F) * F(c.scale)).astype(F)
        return rng, Batch(s, np.concatenate(ys).astype(F), cu, order, c.L)
    counts = valid_counts(c)
    B = len(counts)
    s = rng.standard_normal((B, c.L))
    y = rng.integers(0, 5, (B, c.L)).astype(np.float64)
    for b, nv in enumerate(counts):
        if b == 3:
            s[b] = np.round(s[b] * 4) / 4                        # quantised: many exact ties
        elif nv >= 2:
            s[b, nv - 1] = s[b, 0]
        if b == 1 and B == 4:
            y[b] = 0                                           # maxDCG clamp
        if c.low_tail and nv == c.L and c.L >= 3:              # the last item: label 0, LOW_TAIL_GAP below every other score -- it stands
            s[b, nv - 2] = s[b, 0]                             # before nobody in either ranking, and every pair with it is near saturation
            s[b, nv - 1], y[b, nv - 1] = s[b, :nv - 1].min() - LOW_TAIL_GAP / c.scale, 0
        y[b, nv:] = float(PAD)
    return rng, Batch((s.astype(F) * F(c.scale)).astype(F), y.astype(F))


def perm_of(c):
    if c.par == "identity":
        return np.arange(c.L, dtype=np.int64)
    return np.random.default_rng([c.L, 5]).permutation(c.L).astype(np.int64)


def batch_divisor(c, bt):
    return float(bt.B)


def _ref(c, bt, strict):
    if c.loss == "listnet":
        return listnet_ref(bt, EPS, batch_divisor(c, bt))
    if c.loss == "listmle":
        return listmle_ref(bt, perm_of(c), EPS, batch_divisor(c, bt))
    if c.loss == "approxndcg":
        return approxndcg_ref(bt, EPS, c.par, batch_divisor(c, bt), strict=strict)
    return lambdaloss_ref(bt, EPS, c.par, strict=strict)


_REFS = {}


@functools.lru_cache(maxsize=None)
def _inputs(key):
    """the batch of every case that shares (loss, layout, L, scale, order) -- and, for the guarded losses, the repaired one"""
    c = [c for c in CASES if _key(c) == key][0]
    rng, bt = _draw(c)
    if c.loss in ("approxndcg", "lambdaloss"):
        pars = sorted({d.par for d in CASES if _key(d) == key}, key=repr)
        for _ in range(REPAIR_ROUNDS + 1):
            refs = {par: _ref(c._replace(par=par), bt, False) for par in pars}
            bad = set().union(*[r["violations"] for r in refs.values()])
            if not bad:
                _REFS.update({(key, par): r for par, r in refs.items()})       # of the final inputs: reference() need not repeat them
                break
            for b, i in sorted(bad):
                v = F(F(rng.standard_normal()) * F(c.scale))
                if bt.ragged:
                    bt.s[bt.cu[b] + i] = v
                else:
                    bt.s[b, i] = v
    bt.s.setflags(write=False), bt.y.setflags(write=False)
    return bt


def _key(c):
    return (c.loss, c.layout, c.L, c.scale, c.order, c.low_tail)


def inputs(c):
    """the case's Batch: scores N(0, 1) x scale in fp32, labels 0..4, exact ties (a slate's last valid score repeats its first; one
    slate in quarters), padded tails of different lengths (one fully padded slate, one all-zero slate), repaired against the guard"""
    return _inputs(_key(c))


@functools.lru_cache(maxsize=None)
def reference(c):
    """the fp64 reference of a case (asserting the branch guard), computed once"""
    bt = inputs(c)
    ref = _REFS.get((_key(c), c.par))
    if ref is None:
        return _ref(c, bt, True)
    assert not ref["violations"], "%s: a clamp decision is inside its band for items %s" % (c.name, ref["violations"][:8])
    return ref


def transcription(c, wrong=None):
    bt = inputs(c)
    if c.loss == "listnet":
        return listnet_f32(bt, EPS, batch_divisor(c, bt), wrong)
    if c.loss == "listmle":
        return listmle_f32(bt, perm_of(c), EPS, batch_divisor(c, bt), wrong)
    if c.loss == "approxndcg":
        return approxndcg_f32(bt, EPS, c.par, batch_divisor(c, bt), wrong)
    return lambdaloss_f32(bt, EPS, c.par, wrong)


WRONG = dict(listnet=LISTNET_WRONG, listmle=LISTMLE_WRONG, approxndcg=APPROX_WRONG, lambdaloss=LAMBDA_WRONG)


def checks(c, got, ref=None):
    """{output: (got, ref, bar)} of the floating-point outputs"""
    ref = reference(c) if ref is None else ref
    out = dict(grad=(got["grad"], ref["grad"], ref["bar_grad"]), per=(got["per"], ref["per"], ref["bar_per"]))
    if not (isinstance(ref["loss"], float) and np.isnan(ref["loss"])):
        out["loss"] = (got["loss"], ref["loss"], ref["bar_loss"])
    return out


def exact_ok(c, got, ref=None):
    """the outputs that are compared bit for bit: padded entries 0, the pair count, the orders; NaN loss where the selection is empty"""
    ref = reference(c) if ref is None else ref
    ok = not np.asarray(got["grad"])[ref["zero"]].any()
    if "order" in ref:
        ok = ok and np.array_equal(got["order"], ref["order"])
    if "count" in ref:
        ok = ok and float(got["count"]) == ref["count"]
    if isinstance(ref["loss"], float) and np.isnan(ref["loss"]):
        ok = ok and bool(np.isnan(got["loss"]))
    return bool(ok)


def applies(c, wrong):
    """None if the defect can show on this case, else why it cannot"""
    p = c.par
    if wrong == "row0_off_by_one" and c.layout != "ragged":
        return "the padded layout has no cu_seqlens"
    if c.L < 2 and (wrong != "row0_off_by_one"):
        return "one item has no partner and a gradient of 0"
    if wrong == "lq_rounded_down" and c.layout == "padded" and c.L % 4 == 0:
        return "four whole quarters: nothing is dropped"
    if c.loss == "lambdaloss":
        kk = c.L if (p.k <= 0 or p.k > c.L) else p.k
        if wrong == "rj_gt_kk" and kk >= c.L:
            return "no valid item has rank kk"
        if wrong == "maxdcg_all_ranks" and (kk >= c.L or p.scheme in (0, 5, 6, 7)):
            return "no cut, or a scheme without gains"
        if wrong == "discount_at_rank" and p.scheme in (0, 5, 6, 7):
            return "a scheme without gains"
        if wrong == "diag_grad_kept" and p.scheme != ALL_PAIRS:
            return "only ndcgLoss1 selects the diagonal"
        if wrong == "mu_dropped" and p.scheme != 4:
            return "only ndcgLoss2PP has mu"
        if wrong == "mean_per_slate" and not p.mean:
            return "sum reduction"
        if wrong in ("clamp_sig_not_zeroed", "clamp_wl_not_zeroed", "bwd_from_one_minus") and c.scale == 1:
            return "no pair reaches a clamp at N(0, 1) scores"
        if wrong == "padded_counted" and c.layout == "ragged":
            return "no padded items"
    if c.loss == "approxndcg":
        if wrong == "clamp_c_not_zeroed" and c.scale == 1:
            return "no pair reaches a clamp at N(0, 1) scores"
        if wrong == "alpha_dropped_in_grad" and c.par == 1.0:
            return "alpha 1"
    if c.loss == "listmle" and wrong == "scan_base_by_subtraction" and (-(-c.L // block_threads("listmle", c.L)) < 2 or c.scale == 1):
        return "a chunk of one item, or no entry far below its chunk's end at N(0, 1) scores"
    return None
