"""fp64 references, a-priori entrywise bars, fp32 transcriptions and the case table of the slate-resident FC + ListNet training step
(allrank_amd/csrc/ltrx_fcstep.hip: ltrx_fc_listnet_step and the opt-in ltrx_fc_linear_listnet_step)  --  TEST INFRASTRUCTURE, plain
numpy, needs no GPU.

The contract is STAGEWISE.  A call can write hidden_out, scores, dscores and grads (+ params, exp_avg, exp_avg_sq with Adam); every
stage is compared with an fp64 reference fed with the KERNEL'S OWN upstream output (``stages``), so that every bar is a short
first-order bound and a defect cannot hide behind the conditioning of a later stage.  u = 2^-24, gam(k) = k u / (1 - k u) (also for
a real k), P = step_ref.P_LIBM (expf / logf at 1 ulp <= 2 u), FLT_MIN where a result may be denormal.  The first addition to 0.f of a
chain is exact and still counted; a fused multiply-add only removes a rounding.  No bar holds a measured number.

Launch shape.  nwg = min(B, cus) workgroups; workgroup g owns the slates g, g + nwg, ...: nsl = ceil(B / nwg) at most.  MFMA kernel:
nhb = max(2, ceil(H / 16)); wave (hb, rh) owns hidden units 16 hb .. +15 and slate rows 128 rh .. +127, in tile pairs of 32 rows:
ntp(rh) = the pairs that start below L.  k_red, the chain of ltrx_fc_reduce_kernel: a thread adds every 64th partial, ceil(nwg / 64),
then two 8-way levels of 7 additions: k_red = ceil(nwg / 64) + 14.

ltrx_fc_listnet_step
  hidden   the fp64 sum of EXACTLY the issued products x_lo w_hi + x_hi w_lo + x_hi w_hi (hi = bf16(.), lo = bf16(. - hi): each product
           exact in fp32 and fp64), + b1, ReLU.  An MFMA's 32 products are counted as a sequential chain (the order inside the
           instruction is not documented); 3 MFMAs per K-step of 32 features, nks = ceil(F / 32) K-steps, then the bias:
               bar_hidden = gam(3 * 32 * nks + 1) (|x_lo| |w_hi|^T + |x_hi| |w_lo|^T + |x_hi| |w_hi|^T + |b1|)
           (the sum of the absolute values of the issued terms: within 1 + 2^-7 of |x| |W1|^T + |b1|).  ReLU is 1-Lipschitz: the same
           bar after it, no entry excluded.  Pattern: hidden_kernel > 0 must equal pre_ref > 0 wherever |pre_ref| > bar_hidden.
           Split error (CPU, once per case): |issued products - x W1^T| <= SPLIT_BOUND[0] |x| |W1|^T (tests/test_split_bf16_cpu.py).
  scores   fp64 sum_h hidden_kernel w_out + b_out.  One product rounding, the 4 levels of the 16-lane DPP sum, then b_out and the
           nhb partials added in order:          bar_s = gam(5 + nhb) (sum_h |hidden_kernel w_out| + |b_out|)
  ListNet  (listnet_rows; listNet.py:8-30) at the kernel's fp32 scores s; val = not padded, a_i = M - s_i >= 0, A = max a_i (likewise
           ay, AY for the labels).  e_i = expf(s_i - m_w) exp-combined with expf(m_w - M): the two subtractions move the argument by
           u a_i in all, the two expf by 2 P u; the wave sum 6 levels, the product with the factor 1, the four-wave sum 4:
               rel(S) = (A + 2 P + 11) u;  1 / S one more;  P_i = expf(s_i - M) (1 / S): a_i + P, the product 1:
               bar_P = gam(a_i + A + 3 P + 13) P_i + FLT_MIN          (T_i likewise with ay, AY)
           rr = P / (P + eps): d rr / dP = eps / (P + eps)^2 is decreasing, so with P_lo = max(P - bar_P, 0)
               bar_rr = (1 + gam(2)) bar_P eps / (P_lo + eps)^2 + gam(2) rr       (the addition and the division)
           t = T rr: bar_t = T bar_rr + rr bar_T + bar_T bar_rr + u (T + bar_T) (rr + bar_rr)
           R = sum t, non-negative terms, 6 wave levels + (a + b) + (c + d):  bar_R = (1 + gam(8)) sum bar_t + gam(8) R
           g = (P R - T rr) inv_div.  The scale is the sum of the absolute values of the terms that cancel, P R + T rr; roundings:
           the product P R, the subtraction, the product with inv_div and inv_div = fl(1 / batch_divisor) itself: 4
               bar_g = inv_div ((1 + gam(4)) (P bar_R + R bar_P + bar_P bar_R + bar_t) + gam(4) (P R + T rr))
           padded slots and every slot of a fully padded slate: exactly 0.
           loss of a slate, -sum T log(P + eps): q = P + eps, bar_q = bar_P + u (q + bar_P); logf moves by the relative error of its
           argument and P u of itself: bar_lg = d + P u (|log q| + d), d = bar_q / (q - bar_q);
               bar_lt = T bar_lg + |log q| bar_T + bar_T bar_lg + u (T + bar_T) (|log q| + bar_lg);  the 8 levels as for R.
           loss = sum over slates / batch_divisor (a fully padded slate: 0, the engine's definition): the chain of a workgroup's
           slates nsl, k_red, the product with inv_div and inv_div:  bar_loss = inv_div ((1 + gam(k)) sum bar + gam(k) sum |.|),
           k = nsl + k_red + 2.
  backward dh = fl(dscore_kernel w_out) where hidden_kernel > 0 (ReLU), else 0: ONE fp32 product, reproduced bit for bit (dh_exact).
           dW1 against the fp64 sum of exactly the issued products x_lo dh_hi + x_hi dh_lo + x_hi dh_hi.  The chain of an entry: the
           accumulator of wave (hb, rh) takes 3 MFMAs of 32 rows per tile pair and slate, 96 ntp(rh) nsl; the add of the two row
           halves 1; k_red.  Per row half, on the absolute sums of that half's issued products:
               bar_dW1 = sum_rh gam(96 ntp(rh) nsl + 1 + k_red) S_rh          (never the total row count B L)
           dh is formed in registers as g0 = dscore w_out and split at once, hi = bf16(g0), lo = bf16(g0 - hi): the compiler may fuse
           the product into that subtraction (fma(dscore, w_out, -hi): allowed, and what the instantiations without ReLU do; with
           ReLU the select stands in between).  lo is then the bf16 of the rest of the EXACT product and differs from the lo of
           the rounded one by a bf16 ulp of lo (2^-17 |dh|) where the rest lies within u |dh| of a rounding boundary (dh_lo_fused:
           a handful of elements per case, all of one hidden unit's row of dW1 off by 2e-6 when a heavy row is among them).
           Either is a correct split of the same dh, and a launch takes one of them throughout: WITHOUT ReLU dW1 is held to
           the SAME bar around the emulation with the rounded product's lo or, as a whole tensor, around the one with the fused
           lo; WITH ReLU, where the fusion is impossible, only around the rounded product's.
           d w_out = sum dscore hidden_kernel: a lane adds the 8 rows it holds of a tile pair, 8 ntp nsl, the product 1, two
           shuffles over the four row groups 2, the halves 1:     gam(8 ntp nsl + 4 + k_red) sum |dscore hidden|   per half
           d b1 = sum dh (a fused product adds the exact one: 1):  gam(8 ntp nsl + 4 + k_red) sum |dh|              per half
           d b_out = sum dscore: a lane's nsl slates, 6 wave levels, (a + b) + (c + d):  gam(nsl + 8 + k_red) sum |dscore|
           The H4 padding slots of the flat gradient are exactly 0.
  Adam     params, exp_avg, exp_avg_sq against step_ref.adam_ref under step_ref.adam_bar, driven by the kernel's gradients, t =
           the device step count + 1 (bumped by exactly 1).

ltrx_fc_linear_listnet_step (fp32 FMAs, no split): score = x . v + c, v = W1^T w_out, c = w_out . b1 + b_out
  v        768 / F groups of threads take chunk = ceil(H / ngrp) hidden units each in order (product + addition), then the ngrp
           group sums in order:                                   bar_v = gam(chunk + ngrp) V,  V = |w_out|^T |W1|
  c        b_out and the H products in order:                     bar_c = gam(H + 1) C,  C = |b_out| + sum |w_out b1|
  scores   the partial-dot table (stride 37): (x0 v0 + x1 v1) + (x2 v2 + x3 v3) is 3 roundings, then c and the nc4 = F / 4 partial
           dots in order:   bar_s = |x| bar_v + gam(3 + nc4) |x| (V + bar_v) + (1 + gam(nc4)) bar_c + gam(nc4) C
  ListNet  the same routine, the same stage.
  grads    from the kernel's dscores d: u = sum d x, D = sum d.  A thread holds the rows r0 + rpt k of its column group (rpt = 768 //
           nc4 rows per pass, ceil(L / rpt) passes) and adds d x over them and its nsl slates; the rpt row groups are added in
           order; ltrx_fc_linear_finish_kernel re-reduces the nwg slabs in ng = min(1024 // nc, 16) groups (nc = (F + 4 + H4) / 4):
           a group adds every ng-th slab, then the ng sums in order:  k_fin = ceil(nwg / ng) + ng
               k_u = ceil(L / rpt) nsl + 1 + rpt;   bar_u = gam(k_u + k_fin) sum |d x|;   bar_D = gam(nsl + 8 + k_fin) sum |d|
           dW1 = w_out (x) u (the w_out SNAPSHOT of the step): one product: |w_out| bar_u + u (|w_out| (|u| + bar_u))
           db1 = D w_out likewise; db_out = D.
           dw_out = W1 u + D b1 is formed PER WORKGROUP from its fp32 u and D (8 slices of ceil(F / 8) features in order, the 8
           slices in order, the product b1 D and its addition: ceil(F / 8) + 10) and re-reduced with the slab:
               bar_dwout = gam(k_u + ceil(F / 8) + 10 + k_fin) |W1| sum |d x| + gam(nsl + 10 + k_fin) |b1| sum |d|
  Adam     the same stage.

fp32 transcriptions (fc_f32, lin_f32) follow one fixed summation order with the kernels' structure (workgroup, row half, tile pair,
slab, reduce groups) and take ``wrong=`` one-line defects; DEFECTS names, for each, the cases on which it must leave a bar
(tests/test_fcstep_ref_cpu.py shows both directions).  To find the cases that catch a defect applied to the kernel by hand: its line in
DEFECTS says what it is in the source, ``applies`` returns None for every case of the table on which it must fail.
"""
import os
import re
import zlib
from collections import namedtuple

import numpy as np

from tests.gemm_ref import SPLIT_BOUND, U16, U32, split  # noqa: F401  (U16, U32: re-exported)
from tests.step_ref import F, FLT_MIN, ONE, P_LIBM, U, _wave_sum, adam_bar, adam_f32, adam_ref, f64, gam, over, w, worst  # noqa: F401

assert U == U32
PAD = -1.0
# restated from csrc/ltrx_fcstep.hip; tests/test_fcstep_ref_cpu.py holds them to the source (source_constants)
FC_ROWS, FC_MAXF, FC_MAXH, FC_NLD = 256, 144, 96, 12
FL_KSMALL, FL_KMAX, FL_PSTRIDE = 11, 13, 37
WS_WG_CAP = 1024
CPU_CUS = 256
ADAM = dict(lr=3e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.01)


def source_constants():
    """the same numbers and host predicates read from the source text"""
    here = os.path.dirname(os.path.abspath(__file__))
    src = open(os.path.join(here, "..", "allrank_amd", "csrc", "ltrx_fcstep.hip")).read()

    def find(pat, restated):
        m = re.search(pat, src)
        assert m, ("csrc/ltrx_fcstep.hip no longer holds the text /%s/: re-read the source there and re-sync %s in tests/fcstep_ref.py "
                   "(and this pattern)" % (pat, restated))
        return m

    num = lambda pat, restated: int(find(pat, restated).group(1))      # noqa: E731
    find(r"const int nhb = \(H \+ 15\) / 16 < 2 \? 2 : \(H \+ 15\) / 16;", "nhb_of (ltrx_fc_listnet_step's block size)")
    find(r"const bool full = F > 128;", "kernel_name (the FULL instantiations)")
    find(r"for \(int g = gq; g < nwg; g \+= 64\)", "k_red and reduce_f32 (ltrx_fc_reduce_kernel's 64 groups)")
    find(r"return B < cus \? B : cus;", "nwg_of (fc_workgroups)")
    find(r"const int ng = \(1024 / nc\) < 16 \? \(1024 / nc\) : 16;", "k_fin and lin_f32 (ltrx_fc_linear_finish_kernel's groups)")
    return dict(rows=num(r"constexpr int FC_ROWS = (\d+);", "FC_ROWS"), maxf=num(r"constexpr int FC_MAXF = (\d+);", "FC_MAXF"),
                maxh=num(r"constexpr int FC_MAXH = (\d+);", "FC_MAXH"), nld=num(r"constexpr int FC_NLD = (\d+);", "FC_NLD"),
                kmax=num(r"constexpr int FL_KMAX = (\d+);", "FL_KMAX"), pstride=num(r"constexpr int FL_PSTRIDE = (\d+);", "FL_PSTRIDE"),
                ksmall=num(r"if \(\(L \+ rpt - 1\) / rpt <= (\d+)\)", "FL_KSMALL and lin_shape (the linear kernel's switch)"),
                ws_cap=num(r"const size_t nwg = \(size_t\)\(B < (\d+) \? B : \1\);", "WS_WG_CAP and ws_bytes"))


# ---------------------------------------------------------------------------------------------------------------------------------
# the host's dispatch, restated
# ---------------------------------------------------------------------------------------------------------------------------------
def supported(L, Fn, H):
    return 0 < L <= FC_ROWS and 0 < Fn <= FC_MAXF and Fn % 4 == 0 and 0 < H <= FC_MAXH


def layout(Fn, H):
    """(off_w1, off_b1, off_wout, off_bout, nflat) of the flat parameter / gradient buffer"""
    H4 = (H + 3) // 4 * 4
    return 0, H * Fn, H * Fn + H4, H * Fn + 2 * H4, H * Fn + 2 * H4 + 4


def nwg_of(B, cus):
    return min(B, cus)


def nhb_of(H):
    return max(2, -(-H // 16))


def ntp_of(L, rh):
    return int(np.clip(-(-(L - 128 * rh) // 32), 0, 4))


def k_red(nwg):
    return -(-nwg // 64) + 14


def lin_shape(L, Fn):
    """(rows per pass, passes, KMAX of the instantiation)"""
    rpt = 768 // (Fn // 4)
    passes = -(-L // rpt)
    return rpt, passes, FL_KSMALL if passes <= FL_KSMALL else FL_KMAX


def k_fin(nwg, Fn, H):
    nc = (Fn + 4 + (H + 3) // 4 * 4) // 4
    ng = min(1024 // nc, 16)
    return -(-nwg // ng) + ng


def ws_bytes(kind, B, Fn, H):
    """what *_workspace_bytes promises (an upper bound without a device query)"""
    if kind == "fc":
        return min(B, WS_WG_CAP) * (layout(Fn, H)[4] + 4) * 4
    return (min(B, WS_WG_CAP) * (Fn + 4 + FC_MAXH) + FC_MAXH) * 4


def ws_used(kind, B, Fn, H, cus):
    """the extent the kernels may actually write"""
    if kind == "fc":
        return nwg_of(B, cus) * (layout(Fn, H)[4] + 4) * 4
    return (nwg_of(B, cus) * (Fn + 4 + (H + 3) // 4 * 4) + H) * 4


def kernel_name(c):
    if c.kind == "fc":
        return "ltrx_fc_listnet_kernel<%s, %s>" % ("true" if c.act else "false", "true" if c.F > 128 else "false")
    return "ltrx_fc_linear_listnet_kernel<%d>" % lin_shape(c.L, c.F)[2]


ALL_KERNELS = (["ltrx_fc_listnet_kernel<%s, %s>" % (r, f) for r in ("false", "true") for f in ("false", "true")]
               + ["ltrx_fc_linear_listnet_kernel<%d>" % k for k in (FL_KSMALL, FL_KMAX)])


def unpack(params, Fn, H):
    _, ob1, owo, obo, _ = layout(Fn, H)
    p = np.asarray(params)
    return p[:H * Fn].reshape(H, Fn), p[ob1:ob1 + H], p[owo:owo + H], p[obo]


def _split64(a):
    hi, lo, _ = split(a, 2)
    return f64(hi), f64(lo)


# ---------------------------------------------------------------------------------------------------------------------------------
# stage references and bars
# ---------------------------------------------------------------------------------------------------------------------------------
def hidden_ref(x, params, H, relu):
    """(hidden, pre-activation, bar, |x| |W1|^T + |b1| and the true x W1^T + b1 for the split bound) of [B, L, F] features"""
    B, L, Fn = x.shape
    W1, b1, _, _ = unpack(params, Fn, H)
    x2 = np.asarray(x, F).reshape(B * L, Fn)
    xh, xl = _split64(x2)
    wh, wl = _split64(W1)
    pre = xl @ wh.T + xh @ wl.T + xh @ wh.T + f64(b1)
    S = np.abs(xl) @ np.abs(wh).T + np.abs(xh) @ np.abs(wl).T + np.abs(xh) @ np.abs(wh).T + np.abs(f64(b1))
    bar = gam(96 * (-(-Fn // 32)) + 1) * S
    true = f64(x2) @ f64(W1).T + f64(b1)
    scale = np.abs(f64(x2)) @ np.abs(f64(W1)).T
    sh = (B, L, H)
    return (np.maximum(pre, 0.0) if relu else pre).reshape(sh), pre.reshape(sh), bar.reshape(sh), scale.reshape(sh), true.reshape(sh)


def scores_ref(hidden_k, params, Fn, H):
    _, _, wo, bo = unpack(params, Fn, H)
    h = f64(hidden_k)
    return h @ f64(wo) + float(bo), gam(5 + nhb_of(H)) * (np.abs(h) @ np.abs(f64(wo)) + abs(float(bo)))


def lin_scores_ref(x, params, H):
    B, L, Fn = x.shape
    W1, b1, wo, bo = (f64(t) for t in unpack(params, Fn, H))
    ngrp, nc4 = 768 // Fn, Fn // 4
    chunk = -(-H // ngrp)
    v, V = wo @ W1, np.abs(wo) @ np.abs(W1)
    bar_v = gam(chunk + ngrp) * V
    c, C = wo @ b1 + bo, np.abs(bo) + np.abs(wo * b1).sum()
    bar_c = gam(H + 1) * C
    ax = np.abs(f64(x))
    bar = ax @ bar_v + gam(3 + nc4) * (ax @ (V + bar_v)) + (1 + gam(nc4)) * bar_c + gam(nc4) * C
    return f64(x) @ v + c, bar


def listnet_ref(s, y, eps, div):
    """dict(g, bar_g, loss, bar_loss (per slate, before / batch_divisor), P) at the fp32 scores s [B, L]"""
    s, y, eps, inv = f64(s), f64(y), w(eps), 1.0 / w(div)
    val = y != PAD
    some = val.any(1, keepdims=True)

    def softmax(t):
        m = np.where(some, np.where(val, t, -np.inf).max(1, keepdims=True), 0.0)
        a = np.where(val, m - t, 0.0)
        e = np.where(val, np.exp(-a), 0.0)
        p = e / np.where(some, e.sum(1, keepdims=True), 1.0)
        return p, np.where(val, gam(a + a.max(1, keepdims=True) + 3 * P_LIBM + 13) * p + FLT_MIN, 0.0)

    with np.errstate(invalid="ignore"):
        P, bar_P = softmax(np.where(val, s, 0.0))
        T, bar_T = softmax(np.where(val, y, 0.0))
    rr = P / (P + eps)
    P_lo = np.maximum(P - bar_P, 0.0)
    bar_rr = (1 + gam(2)) * bar_P * eps / (P_lo + eps) ** 2 + gam(2) * rr
    t = T * rr
    bar_t = T * bar_rr + rr * bar_T + bar_T * bar_rr + U * (T + bar_T) * (rr + bar_rr)
    R = t.sum(1, keepdims=True)
    bar_R = (1 + gam(8)) * bar_t.sum(1, keepdims=True) + gam(8) * R
    g = (P * R - t) * inv
    bar_g = inv * ((1 + gam(4)) * (P * bar_R + R * bar_P + bar_P * bar_R + bar_t) + gam(4) * (P * R + t))
    q = P + eps
    bar_q = bar_P + U * (q + bar_P)
    assert not (bar_q >= q).any()                          # (a NaN score is outside every bar anyway)
    lg = np.abs(np.log(q))
    d = bar_q / (q - bar_q)
    bar_lg = d + P_LIBM * U * (lg + d)
    lt = np.where(val, T * np.log(q), 0.0)
    bar_lt = np.where(val, T * bar_lg + lg * bar_T + bar_T * bar_lg + U * (T + bar_T) * (lg + bar_lg), 0.0)
    loss = -lt.sum(1)
    bar_loss = (1 + gam(8)) * bar_lt.sum(1) + gam(8) * np.abs(lt).sum(1)
    return dict(g=np.where(val, g, 0.0), bar_g=np.where(val, bar_g, 0.0), loss=loss, bar_loss=bar_loss, P=P, val=val)


def loss_ref(ln, div, B, cus):
    k = -(-B // nwg_of(B, cus)) + k_red(nwg_of(B, cus)) + 2
    inv = 1.0 / w(div)
    return ln["loss"].sum() * inv, inv * ((1 + gam(k)) * ln["bar_loss"].sum() + gam(k) * np.abs(ln["loss"]).sum())


def lin_loss_ref(ln, div, B, Fn, H, cus):
    k = -(-B // nwg_of(B, cus)) + k_fin(nwg_of(B, cus), Fn, H) + 2
    inv = 1.0 / w(div)
    return ln["loss"].sum() * inv, inv * ((1 + gam(k)) * ln["bar_loss"].sum() + gam(k) * np.abs(ln["loss"]).sum())


def dh_exact(dsc_k, hidden_k, params, Fn, H, relu):
    """the fp32 dh the kernel forms: one product, masked with the kernel's own pattern"""
    _, _, wo, _ = unpack(params, Fn, H)
    dh = (np.asarray(dsc_k, F)[:, :, None] * np.asarray(wo, F)[None, None, :]).astype(F)
    return np.where(np.asarray(hidden_k) > 0, dh, F(0)) if relu else dh


def dh_lo_fused(dsc_k, dh, params, Fn, H):
    """the lo term of dh when the compiler fuses the product into the split's subtraction: bf16(fl(dscore w_out - hi)) with the product
    exact inside the fma (it is exact in fp64, and so is the difference)"""
    _, _, wo, _ = unpack(params, Fn, H)
    hi = f64(split(dh, 2)[0])
    rest = (f64(dsc_k)[:, :, None] * f64(wo)[None, None, :] - hi).astype(F)
    return f64(split(np.where(dh == 0, F(0), rest), 1)[0])


def fc_grads_ref(x, params, H, relu, hidden_k, dsc_k, cus):
    """(flat gradient, flat bar, dW1 with the fused-product lo term of dh) in fp64 from the kernel's hidden and dscores"""
    B, L, Fn = x.shape
    _, ob1, owo, obo, nflat = layout(Fn, H)
    nw = nwg_of(B, cus)
    nsl, kr = -(-B // nw), k_red(nw)
    dh = dh_exact(dsc_k, hidden_k, params, Fn, H, relu)
    d, h = f64(dsc_k), f64(hidden_k)
    ref, bar, fused = np.zeros(nflat), np.zeros(nflat), np.zeros(nflat)
    lo_fused = dh_lo_fused(dsc_k, dh, params, Fn, H)
    for rh in (0, 1):
        ntp = ntp_of(L, rh)
        if ntp == 0:
            continue
        rows = slice(128 * rh, min(L, 128 * rh + 128))
        n = B * (rows.stop - rows.start)
        xh, xl = _split64(np.asarray(x, F)[:, rows].reshape(n, Fn))
        dhh, dhl = _split64(dh[:, rows].reshape(n, H))
        ref[:H * Fn] += (dhh.T @ xl + dhl.T @ xh + dhh.T @ xh).ravel()
        S = np.abs(dhh).T @ np.abs(xl) + np.abs(dhl).T @ np.abs(xh) + np.abs(dhh).T @ np.abs(xh)
        fused[:H * Fn] += (dhh.T @ xl + lo_fused[:, rows].reshape(n, H).T @ xh + dhh.T @ xh).ravel()
        bar[:H * Fn] += gam(96 * ntp * nsl + 1 + kr) * S.ravel()
        dr, hr = d[:, rows].reshape(n, 1), h[:, rows].reshape(n, H)
        ref[owo:owo + H] += (dr * hr).sum(0)
        bar[owo:owo + H] += gam(8 * ntp * nsl + 4 + kr) * np.abs(dr * hr).sum(0)
        ref[ob1:ob1 + H] += f64(dh[:, rows]).reshape(n, H).sum(0)
        bar[ob1:ob1 + H] += gam(8 * ntp * nsl + 4 + kr) * np.abs(f64(dh[:, rows])).reshape(n, H).sum(0)
    ref[obo] = d.sum()
    bar[obo] = gam(nsl + 8 + kr) * np.abs(d).sum()
    return ref, bar, fused[:H * Fn]


def lin_grads_ref(x, params, H, dsc_k, cus):
    B, L, Fn = x.shape
    _, ob1, owo, obo, nflat = layout(Fn, H)
    W1, b1, wo, _ = (f64(t) for t in unpack(params, Fn, H))
    nw = nwg_of(B, cus)
    nsl, kf = -(-B // nw), k_fin(nw, Fn, H)
    rpt, passes, _ = lin_shape(L, Fn)
    d = f64(dsc_k).reshape(B * L, 1)
    x2 = f64(x).reshape(B * L, Fn)
    u, ua = (d * x2).sum(0), np.abs(d * x2).sum(0)
    D, Da = d.sum(), np.abs(d).sum()
    k_u = passes * nsl + 1 + rpt
    bar_u, bar_D = gam(k_u + kf) * ua, gam(nsl + 8 + kf) * Da
    ref, bar = np.zeros(nflat), np.zeros(nflat)
    aw = np.abs(wo)
    ref[:H * Fn] = np.outer(wo, u).ravel()
    bar[:H * Fn] = (np.outer(aw, bar_u) + U * np.outer(aw, np.abs(u) + bar_u)).ravel()
    ref[ob1:ob1 + H] = D * wo
    bar[ob1:ob1 + H] = aw * bar_D + U * aw * (abs(D) + bar_D)
    ref[owo:owo + H] = W1 @ u + D * b1
    bar[owo:owo + H] = gam(k_u + -(-Fn // 8) + 10 + kf) * (np.abs(W1) @ ua) + gam(nsl + 10 + kf) * np.abs(b1) * Da
    ref[obo], bar[obo] = D, bar_D
    return ref, bar


def relu_undecidable(pre, bar):
    return np.abs(pre) <= bar


def stages(c, X, got, cus):
    """[(stage, got, reference, bar)] of one call's outputs ``got``: dict(hidden (MFMA kernel only, may be None), scores, dscores (may be
    None), loss, grads [, params, exp_avg, exp_avg_sq, step with Adam]).  Exact requirements have a bar of 0."""
    x, y, p0 = X["x"], X["y"], X["params"]
    B, L, Fn = x.shape
    H = c.H
    _, ob1, owo, obo, nflat = layout(Fn, H)
    out = []
    if c.kind == "fc":
        hid, pre, bar_h, _, _ = hidden_ref(x, p0, H, c.act)
        out.append(("hidden", got["hidden"], hid, bar_h))
        if c.act:
            und = relu_undecidable(pre, bar_h)
            out.append(("relu pattern", ((np.asarray(got["hidden"]) > 0) != (pre > 0)) & ~und, np.zeros(pre.shape), np.zeros(pre.shape)))
        out.append(("scores",) + (got["scores"],) + scores_ref(got["hidden"], p0, Fn, H))
    else:
        out.append(("scores",) + (got["scores"],) + lin_scores_ref(x, p0, H))
    ln = listnet_ref(got["scores"], y, c.eps, c.div)
    dsc = got["dscores"]
    out.append(("dscores", dsc, ln["g"], ln["bar_g"]))
    out.append(("loss", np.asarray(got["loss"]).reshape(1)) + tuple(np.reshape(t, 1) for t in (
        loss_ref(ln, c.div, B, cus) if c.kind == "fc" else lin_loss_ref(ln, c.div, B, Fn, H, cus))))
    if c.kind == "fc":
        gref, gbar, fused = fc_grads_ref(x, p0, H, c.act, got["hidden"], dsc, cus)
        g = np.asarray(got["grads"])
        if not c.act and worst(g[:H * Fn], fused, gbar[:H * Fn]) < worst(g[:H * Fn], gref[:H * Fn], gbar[:H * Fn]):
            gref[:H * Fn] = fused                               # the instantiation splits the exact product: see the module docstring
    else:
        gref, gbar = lin_grads_ref(x, p0, H, dsc, cus)
    g = np.asarray(got["grads"])
    for name, sl in (("dW1", slice(0, H * Fn)), ("db1", slice(ob1, ob1 + H)), ("dw_out", slice(owo, owo + H)), ("db_out", slice(obo, obo + 1))):
        out.append((name, g[sl], gref[sl], gbar[sl]))
    padding = np.ones(nflat, bool)
    for sl in (slice(0, H * Fn), slice(ob1, ob1 + H), slice(owo, owo + H), slice(obo, obo + 1)):
        padding[sl] = False
    out.append(("grads padding", g[padding], np.zeros(int(padding.sum())), np.zeros(int(padding.sum()))))
    if c.adam:
        kw = dict(ADAM, decoupled=int(c.adam == "adamw"), t=c.t0 + 1)
        ref = adam_ref(p0, g, X["m"], X["v"], **kw)
        bar = adam_bar(p0, g, X["m"], X["v"], **kw)
        for name, a, r, b in zip(("params", "exp_avg", "exp_avg_sq"), (got["params"], got["exp_avg"], got["exp_avg_sq"]), ref, bar):
            out.append(("adam " + name, a, r, b))
        out.append(("step count", np.reshape(got["step"], 1), np.array([c.t0 + 1.0]), np.zeros(1)))
    return out


def ratios(c, X, got, cus):
    """{stage: worst error / bar}"""
    return {name: worst(a, r, b) for name, a, r, b in stages(c, X, got, cus)}


# ---------------------------------------------------------------------------------------------------------------------------------
# fp32 transcriptions
# ---------------------------------------------------------------------------------------------------------------------------------
def _seq(terms, start=None):
    acc = np.zeros_like(terms[0]) if start is None else start
    for t in terms:
        acc = acc + t
    return acc


def listnet_f32(s, y, eps, inv_div, wrong=None):
    """listnet_rows for the slates s, y [B, L]: (g [B, L], the per-slate value added to loss_acc [B])"""
    B, L = s.shape
    eps = F(eps)
    sp, yp = np.zeros((B, FC_ROWS), F), np.full((B, FC_ROWS), PAD, F)
    sp[:, :L], yp[:, :L] = s, y
    val = (yp != F(PAD)) if wrong != "pad_kept" else (np.arange(FC_ROWS) < L)[None, :].repeat(B, 0)
    W = lambda t: t.reshape(B, 4, 64)      # noqa: E731
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        sv, yv = np.where(val, sp, -np.inf).astype(F), np.where(val, yp, -np.inf).astype(F)
        mw, myw = W(sv).max(2), W(yv).max(2)
        if wrong == "label_no_max":
            myw = np.where(np.isfinite(myw), F(0), myw)
        e = np.where(val, np.exp(sv - mw.repeat(64, 1)), F(0)).astype(F)
        f = np.where(val, np.exp(yv - myw.repeat(64, 1)), F(0)).astype(F)
        sw, syw = _wave_sum(W(e)), _wave_sum(W(f))
        M, MY = mw.max(1, keepdims=True), myw.max(1, keepdims=True)
        S, SY = np.zeros((B, 1), F), np.zeros((B, 1), F)
        for k in range(4):
            S = S + np.where(sw[:, k:k + 1] > 0, sw[:, k:k + 1] * np.exp(mw[:, k:k + 1] - M), F(0)).astype(F)
            SY = SY + np.where(syw[:, k:k + 1] > 0, syw[:, k:k + 1] * np.exp(myw[:, k:k + 1] - MY), F(0)).astype(F)
        inv_s = np.where(S > 0, ONE / S, F(0)).astype(F)
        inv_y = np.where(SY > 0, ONE / SY, F(0)).astype(F)
        P = np.where(val, np.exp(sv - M) * inv_s, F(0)).astype(F)
        T = np.where(val, np.exp(yv - MY) * inv_y, F(0)).astype(F)
        if wrong == "eps_outside":
            rr = np.where(P > 0, ONE, F(0)).astype(F)
            lt = np.where(T > 0, T * (np.log(np.where(P > 0, P, ONE)) + eps), F(0)).astype(F)
        else:
            rr = np.where(P > 0, P / (P + eps), F(0)).astype(F)
            lt = np.where(T > 0, T * np.log(P + eps), F(0)).astype(F)
        lw, rw = _wave_sum(W(lt)), _wave_sum(W(T * rr))
        R = ((rw[:, 0] + rw[:, 1]) + (rw[:, 2] + rw[:, 3]))[:, None]
        g = ((P * R - T * rr) * inv_div).astype(F)
        val_loss = (lw[:, 0] + lw[:, 1]) + (lw[:, 2] + lw[:, 3])
    return g[:, :L], val_loss.astype(F)


def reduce_f32(slab, wrong=None):
    """ltrx_fc_reduce_kernel on the partials [nwg, n]"""
    part = np.zeros((64, slab.shape[1]), F)
    for g in range(slab.shape[0]):
        if wrong == "reduce_g64" and g >= 64:
            continue
        part[g % 64] = part[g % 64] + slab[g]
    u = [_seq(list(part[8 * k + 1:8 * k + 8]), part[8 * k]) for k in range(8)]
    return _seq(u[1:], u[0])


FC_WRONG = ("no_xl_wh", "no_cross", "no_xh_dhl", "tail_lo_dropped", "half_chunk_dropped", "rows128_dropped", "first_slate_only",
            "last_twice", "reduce_g64", "relu_ge", "pad_kept", "eps_outside", "label_no_max", "B_divisor")
LIN_WRONG = ("no_D_b1", "odd_last_dropped", "pad_kept", "B_divisor")
# what each defect is in the source
DEFECTS = {
    "no_xl_wh": "forward: the FC_MFMA(fr[1] / fr[3], wh[ks], .) pair (x_lo w_hi) removed",
    "no_cross": "forward: both cross pairs removed, plain bf16 x_hi w_hi",
    "no_xh_dhl": "weight gradient: FC_MFMA(xh, dhl, out[fb]) removed",
    "tail_lo_dropped": "staging or reads of the lo plane's tail panel (features >= 128) lost",
    "half_chunk_dropped": "the W1 fragment loads ask for a whole 8-feature chunk: the last 4 features of an F % 8 == 4 row are zero",
    "rows128_dropped": "the rh = 1 partial is not added in the final combine (rows >= 128 of every slate missing from the gradient)",
    "first_slate_only": "the accumulators are reset per slate and only the first survives (slates b >= gridDim.x missing from the gradient)",
    "last_twice": "a workgroup's last slate enters its accumulators twice",
    "reduce_g64": "ltrx_fc_reduce_kernel reads one partial per thread instead of every 64th (partials g >= 64 missing)",
    "relu_ge": "ReLU backward h >= 0 instead of h > 0",
    "pad_kept": "listnet_rows: val = in_range, the padding test lost",
    "eps_outside": "listnet_rows: log(P) + eps, and rr = 1",
    "label_no_max": "listnet_rows: expf(y) without the label maximum",
    "B_divisor": "inv_div = 1 / B instead of 1 / batch_divisor",
    "no_D_b1": "linear kernel: dw_out share without b1 Dw",
    "odd_last_dropped": "linear kernel: the slate loop runs while b + gridDim.x < B (a workgroup's odd last slate is never processed)",
}
assert set(DEFECTS) == set(FC_WRONG) | set(LIN_WRONG)


def _finish(c, X, out, grads):
    if c.adam:
        p, m, v = adam_f32(X["params"], grads, X["m"], X["v"], decoupled=int(c.adam == "adamw"), t=c.t0 + 1, **ADAM)
        out.update(params=p, exp_avg=m, exp_avg_sq=v, step=F(c.t0 + 1))
    return out


def fc_f32(c, X, cus, wrong=None):
    """the outputs of ltrx_fc_listnet_step in np.float32, in the structure of the source and one fixed order inside an MFMA"""
    x, y, p0 = np.asarray(X["x"], F), np.asarray(X["y"], F), np.asarray(X["params"], F)
    B, L, Fn = x.shape
    H = c.H
    _, ob1, owo, obo, nflat = layout(Fn, H)
    W1, b1, wo, bo = unpack(p0, Fn, H)
    xh, xl, _ = split(x, 2)
    wh, wl, _ = split(W1, 2)
    if wrong == "tail_lo_dropped":
        xl = xl.copy()
        xl[..., 128:] = 0
    if wrong == "half_chunk_dropped" and Fn % 8 == 4:
        wh, wl = wh.copy(), wl.copy()
        wh[:, Fn - 4:], wl[:, Fn - 4:] = 0, 0
    acc = np.zeros((B, L, H), F)
    for ks in range(-(-Fn // 32)):
        sl = slice(32 * ks, min(Fn, 32 * ks + 32))
        if wrong not in ("no_xl_wh", "no_cross"):
            acc = acc + xl[..., sl] @ wh[:, sl].T
        if wrong != "no_cross":
            acc = acc + xh[..., sl] @ wl[:, sl].T
        acc = acc + xh[..., sl] @ wh[:, sl].T
    hid = acc + b1
    if c.act:
        hid = np.maximum(hid, F(0))
    # scores: the product, the 16-lane tree of a block of hidden units, b_out and the blocks in order
    nhb = nhb_of(H)
    prod = np.zeros((B, L, 16 * nhb), F)
    prod[..., :H] = hid * wo
    t = prod.reshape(B, L, nhb, 16)
    for _ in range(4):
        t = t[..., 0::2] + t[..., 1::2]
    sc = _seq([t[:, :, q, 0] for q in range(nhb)], np.full((B, L), bo, F))
    inv_div = ONE / F(B if wrong == "B_divisor" else c.div)
    g, lval = listnet_f32(sc, y, c.eps, inv_div, wrong)
    # backward: per workgroup and row half, tile pair by tile pair
    nw = nwg_of(B, cus)
    dh = g[:, :, None] * wo[None, None, :]
    if c.act:
        dh = np.where(hid >= 0 if wrong == "relu_ge" else hid > 0, dh, F(0))
    dh = dh.astype(F)
    dhh, dhl, _ = split(dh, 2)
    dW = np.zeros((nw, 2, H, Fn), F)
    dwo, db1, dbo, lacc = np.zeros((nw, 2, H), F), np.zeros((nw, 2, H), F), np.zeros(nw, F), np.zeros(nw, F)

    def slate_rows(bs):
        wg = bs % nw
        for rh in ((0,) if wrong == "rows128_dropped" else (0, 1)):
            for kp in range(4):
                R0 = 128 * rh + 32 * kp
                if R0 >= L:
                    continue
                r = slice(R0, min(L, R0 + 32))
                tr = lambda a: a[bs, r].transpose(0, 2, 1)      # noqa: E731
                a = dW[wg, rh] + tr(dhh) @ xl[bs, r]
                if wrong != "no_xh_dhl":
                    a = a + tr(dhl) @ xh[bs, r]
                dW[wg, rh] = a + tr(dhh) @ xh[bs, r]
                for k in range(r.start, r.stop):
                    dwo[wg, rh] = dwo[wg, rh] + g[bs, k, None] * hid[bs, k]
                    db1[wg, rh] = db1[wg, rh] + dh[bs, k]

    for it in range(-(-B // nw)):
        bs = np.arange(it * nw, min(B, (it + 1) * nw))
        dbo[bs % nw] = dbo[bs % nw] + g[bs].sum(1, dtype=F)
        lacc[bs % nw] = lacc[bs % nw] - lval[bs]
        if it >= 1 and wrong == "first_slate_only":
            continue
        slate_rows(bs)
        if wrong == "last_twice":
            slate_rows(bs[bs + nw >= B])
    slab = np.zeros((nw, nflat + 4), F)
    slab[:, :H * Fn] = (dW[:, 0] + dW[:, 1]).reshape(nw, H * Fn)
    slab[:, owo:owo + H] = dwo[:, 0] + dwo[:, 1]
    slab[:, ob1:ob1 + H] = db1[:, 0] + db1[:, 1]
    slab[:, obo], slab[:, nflat] = dbo, lacc
    tot = reduce_f32(slab, wrong)
    out = dict(hidden=hid.astype(F), scores=sc.astype(F), dscores=g, loss=F(tot[nflat] * inv_div), grads=tot[:nflat].copy())
    return _finish(c, X, out, out["grads"])


def lin_f32(c, X, cus, wrong=None):
    """the outputs of ltrx_fc_linear_listnet_step in np.float32 in the order of the source"""
    x, y, p0 = np.asarray(X["x"], F), np.asarray(X["y"], F), np.asarray(X["params"], F)
    B, L, Fn = x.shape
    H = c.H
    H4 = (H + 3) // 4 * 4
    _, ob1, owo, obo, nflat = layout(Fn, H)
    W1, b1, wo, bo = unpack(p0, Fn, H)
    ngrp, nc4 = 768 // Fn, Fn // 4
    chunk = -(-H // ngrp)
    vp = [_seq([wo[n] * W1[n] for n in range(gq * chunk, min(H, gq * chunk + chunk))], np.zeros(Fn, F)) for gq in range(ngrp)]
    v = _seq(vp[1:], vp[0])
    cc = _seq([wo[n] * b1[n] for n in range(H)], F(bo))
    xv = (x * v).reshape(B, L, nc4, 4)
    part = (xv[..., 0] + xv[..., 1]) + (xv[..., 2] + xv[..., 3])
    sc = _seq([part[:, :, q] for q in range(nc4)], np.full((B, L), cc, F))
    inv_div = ONE / F(B if wrong == "B_divisor" else c.div)
    g, lval = listnet_f32(sc, y, c.eps, inv_div, wrong)
    nw = nwg_of(B, cus)
    rpt, passes, _ = lin_shape(L, Fn)
    u4 = np.zeros((nw, rpt, Fn), F)
    dsum, lacc = np.zeros((nw, FC_ROWS), F), np.zeros(nw, F)
    done = np.ones(B, bool)
    for it in range(-(-B // nw)):
        bs = np.arange(it * nw, min(B, (it + 1) * nw))
        if wrong == "odd_last_dropped" and it % 2 == 0:
            bs = bs[bs + nw < B]
            done[it * nw + np.flatnonzero(np.arange(it * nw, min(B, (it + 1) * nw)) + nw >= B)] = False
        wg = bs % nw
        dsum[wg, :L] = dsum[wg, :L] + g[bs]
        lacc[wg] = lacc[wg] - lval[bs]
        for k in range(passes):
            r = np.arange(rpt * k, min(L, rpt * k + rpt))
            u4[wg[:, None], (r - rpt * k)[None, :]] = u4[wg[:, None], (r - rpt * k)[None, :]] + g[bs][:, r, None] * x[bs][:, r]
    uw = _seq(list(u4.transpose(1, 0, 2)[1:]), u4[:, 0])                                    # [nw, F]
    dw_ = _wave_sum(dsum.reshape(nw, 4, 64))
    Dw = (dw_[:, 0] + dw_[:, 1]) + (dw_[:, 2] + dw_[:, 3])
    fchunk = -(-Fn // 8)
    rp = []
    for sl in range(8):
        rp.append(_seq([W1[None, :, f] * uw[:, f, None] for f in range(sl * fchunk, min(Fn, sl * fchunk + fchunk))], np.zeros((nw, H), F)))
    share = _seq(rp[1:], rp[0])
    if wrong != "no_D_b1":
        share = share + b1[None, :] * Dw[:, None]
    ss = Fn + 4 + H4
    slab = np.zeros((nw, ss), F)
    slab[:, :Fn], slab[:, Fn], slab[:, Fn + 1], slab[:, Fn + 4:Fn + 4 + H] = uw, Dw, lacc, share
    ng = min(1024 // (ss // 4), 16)
    ps = [_seq(list(slab[gq::ng]), np.zeros(ss, F)) for gq in range(ng)]
    tot = _seq(ps[1:], ps[0])
    grads = np.zeros(nflat, F)
    grads[:H * Fn] = np.outer(wo, tot[:Fn]).ravel()
    grads[ob1:ob1 + H] = wo * tot[Fn]
    grads[owo:owo + H] = tot[Fn + 4:Fn + 4 + H]
    grads[obo] = tot[Fn]
    sc = sc.astype(F)
    sc[~done] = np.nan                                          # a slate that is never processed leaves its scores unwritten
    g = g.copy()
    g[~done] = np.nan
    out = dict(scores=sc, dscores=g, loss=F(tot[Fn + 1] * inv_div), grads=grads)
    return _finish(c, X, out, grads)


def transcribe(c, X, cus, wrong=None):
    return (fc_f32 if c.kind == "fc" else lin_f32)(c, X, cus, wrong)


# ---------------------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------------------
# B: an int, or (m, a) for m * cus + a.  weights: "init" (uniform +- 1 / sqrt(fan in), as torch.nn.Linear) or "big" (w_out, b_out scaled so
# that the largest |score| is 30).  adam: None, "l2" (torch.optim.Adam with weight decay) or "adamw"; t0: the device step count before the
# call.  div: batch_divisor as a multiple of B.  eps: ListNet's.
Case = namedtuple("Case", "name kind B L F H act weights adam t0 div_mul eps idx")


def _cases():
    out = []

    def add(kind, B, L, Fn, H, act=0, weights="init", adam=None, t0=0, div_mul=1.0, eps=1e-10):
        bname = str(B) if isinstance(B, int) else ("%d cus + %d" % B if B[0] > 1 else "cus + %d" % B[1] if B[1] else "cus")
        name = "%s B %s L %d F %d H %d%s %s%s" % (kind, bname, L, Fn, H, " relu" if act else "", weights,
                                                 "" if adam is None else " %s t0 %d" % (adam, t0))
        out.append(Case(name, kind, B, L, Fn, H, act, weights, adam, t0, div_mul, eps, len(out)))

    # the MFMA kernel: every F, H, L of the list, the four instantiations, the staging loop, the workgroup and reduce-group boundaries
    add("fc", 1, 1, 4, 1, act=0)
    add("fc", 2, 16, 12, 16, act=0, adam="l2", div_mul=2.5)
    add("fc", 3, 17, 36, 17, act=1, adam="adamw", t0=9)
    add("fc", 3, 32, 44, 33, act=0, weights="big", eps=1e-5)
    add("fc", 4, 33, 128, 80, act=1, div_mul=0.5)
    add("fc", 3, 127, 132, 96, act=0, adam="adamw")
    add("fc", 3, 128, 136, 96, act=1, weights="big", adam="l2", t0=9)
    add("fc", 4, 129, 144, 80, act=0, eps=1e-5)
    add("fc", 7, 129, 44, 17, act=1, div_mul=3.0)
    add("fc", 3, 240, 136, 33, act=1, adam="l2")                       # the plain staging loop at 384 threads
    add("fc", 4, 256, 144, 16, act=1, weights="big")                   # ... at 256 threads
    add("fc", 7, 256, 144, 96, act=1, adam="adamw", t0=9, div_mul=2.0)
    add("fc", 7, 240, 136, 96, act=0, weights="big", eps=1e-5)
    for B in (63, 64, 65):
        add("fc", B, 33, 36, 20, act=B % 2, adam=None if B == 64 else "l2", div_mul=1.0 if B == 63 else 1.5)
    add("fc", (1, 0), 33, 36, 20, act=0, adam="adamw")
    add("fc", (1, 1), 33, 36, 20, act=1, div_mul=2.0)
    add("fc", (2, 1), 33, 36, 20, act=1, adam="l2", t0=9)
    add("fc", (1, 1), 17, 132, 17, act=0)
    # the linear kernel: both instantiations at their switch, 1 .. 4 slates per workgroup
    add("lin", 3, 240, 136, 96, adam="l2")
    add("lin", 3, 243, 136, 96, weights="big", eps=1e-5, div_mul=2.0)
    add("lin", 4, 256, 144, 33, adam="adamw", t0=9)
    add("lin", 5, 17, 4, 1)
    add("lin", 6, 129, 44, 17, weights="big", div_mul=0.5)
    add("lin", (1, 0), 16, 12, 16, adam="adamw")
    add("lin", (1, 1), 33, 36, 20, div_mul=2.0)
    add("lin", (2, 1), 33, 36, 20, adam="l2", t0=9)
    add("lin", (3, 1), 33, 36, 20)
    return out


CASES = _cases()
PATTERNS = ("full", "ragged", "interior pad", "one item", "fully padded", "all zero", "big label")


def batch(c, cus):
    return c.B if isinstance(c.B, int) else c.B[0] * cus + c.B[1]


def pattern(c, b):
    return PATTERNS[(b + c.idx) % len(PATTERNS)]


def inputs(c, cus):
    """dict(x [B, L, F], y [B, L], params, m, v [nflat], underflow): features N(0, 1) with columns scaled by 2^[-6, 6] (left as they are
    at padded slots), labels 0 .. 4 with the slate patterns of PATTERNS in rotation ("big label": one label of 100, so that a label
    softmax without its max overflows), and, where a slate has four valid items, one row scaled until its score lies 95 below the
    slate's largest: its P underflows in fp32."""
    B, L, Fn, H = batch(c, cus), c.L, c.F, c.H
    rng = np.random.default_rng([zlib.crc32(c.name.encode()), cus])
    x = (rng.standard_normal((B, L, Fn)) * 2.0 ** rng.integers(-6, 7, (1, 1, Fn))).astype(F)
    y = rng.choice(5, size=(B, L), p=[0.52, 0.32, 0.13, 0.02, 0.01]).astype(F)
    for b in range(B):
        k = pattern(c, b)
        if k == "ragged":
            y[b, max(1, L // 2):] = PAD
        elif k == "interior pad" and L >= 3:
            y[b, L // 3] = PAD
        elif k == "one item":
            y[b, 1:] = PAD
        elif k == "fully padded":
            y[b] = PAD
        elif k == "all zero":
            y[b] = 0
        elif k == "big label":
            y[b, L - 1:] = PAD if L > 1 else y[b, L - 1]
            y[b, 0] = 100
    _, ob1, owo, obo, nflat = layout(Fn, H)
    p = np.zeros(nflat, F)
    uni = lambda n, fan: (rng.uniform(-1, 1, n) / np.sqrt(fan)).astype(F)      # noqa: E731
    p[:H * Fn], p[ob1:ob1 + H], p[owo:owo + H], p[obo] = uni(H * Fn, Fn), uni(H, Fn), uni(H, H), uni(1, H)[0]

    def score64(xx):
        W1, b1, wo, bo = (f64(t) for t in unpack(p, Fn, H))
        pre = f64(xx) @ W1.T + b1
        return (np.maximum(pre, 0) if (c.kind == "fc" and c.act) else pre) @ wo + bo

    valid = y != PAD
    if c.weights == "big" and valid.any():
        k = F(30.0 / np.abs(score64(x)[valid]).max())
        p[owo:owo + H] *= k
        p[obo] *= k
    underflow = False
    cand = np.flatnonzero(valid.sum(1) >= 4)
    if cand.size:
        b = int(cand[0])
        r = int(np.flatnonzero(valid[b])[1])
        others = valid[b].copy()
        others[r] = False
        top = score64(x[b])[others].max()
        for a in [s * 2.0 ** k for k in range(1, 25) for s in (1.0, -1.0)]:
            row = (x[b, r] * F(a)).astype(F)
            if np.isfinite(row).all() and -140 < score64(row[None])[0] - top < -95:
                x[b, r], underflow = row, True
                break
    m, v = np.zeros(nflat, F), np.zeros(nflat, F)
    live = np.zeros(nflat, bool)
    for sl in (slice(0, H * Fn), slice(ob1, ob1 + H), slice(owo, owo + H), slice(obo, obo + 1)):
        live[sl] = True
    m[live] = (1e-3 * rng.standard_normal(int(live.sum()))).astype(F)
    v[live] = ((1e-3 * rng.standard_normal(int(live.sum()))) ** 2).astype(F)
    return dict(x=x, y=y, params=p, m=m, v=v, underflow=underflow, B=B)


CaseR = namedtuple("CaseR", Case._fields + ("div",))


def resolve(c, cus):
    """the case with its batch_divisor on a device of ``cus`` compute units: B * div_mul (not B wherever div_mul != 1)"""
    return CaseR(*c, div=float(batch(c, cus)) * c.div_mul)


# ---------------------------------------------------------------------------------------------------------------------------------
# which defect must show on which case
# ---------------------------------------------------------------------------------------------------------------------------------
def eps_shift_shows(c, X, cus):
    """what `log(P) + eps` for `log(P + eps)` moves, exactly, at the fp64 scores of the inputs: the loss by sum T (log(1 + eps / P) - eps)
    / batch_divisor, rr from P / (P + eps) to 1 and with it every d loss / d score.  Where P is of ordinary size and eps is 1e-10 both are
    below the roundings of the other terms and no bar can tell (as layernorm_ref.tc_shift)"""
    x, p0 = X["x"], X["params"]
    B, L, Fn = x.shape
    W1, b1, wo, bo = (f64(t) for t in unpack(p0, Fn, c.H))
    pre = f64(x) @ W1.T + b1
    s = (np.maximum(pre, 0) if (c.kind == "fc" and c.act) else pre) @ wo + bo
    ln = listnet_ref(s.astype(F), X["y"], c.eps, c.div)
    eps, inv, P, val = w(c.eps), 1.0 / w(c.div), ln["P"], ln["val"]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        Tm = np.where(val, np.exp(np.where(val, f64(X["y"]), 0.0) - np.where(val, f64(X["y"]), -np.inf).max(1, keepdims=True)), 0.0)
        T = np.where(val.any(1, keepdims=True), Tm / np.where(val.any(1, keepdims=True), Tm.sum(1, keepdims=True), 1.0), 0.0)
        dl = np.where(val & (P > 0), T * np.abs(np.log1p(eps / np.where(P > 0, P, 1.0)) - eps), 0.0)
    drr = np.where(val, eps / (P + eps), 0.0)
    dg = np.abs(P * (T * drr).sum(1, keepdims=True) - T * drr) * inv
    kind_loss = loss_ref(ln, c.div, B, cus) if c.kind == "fc" else lin_loss_ref(ln, c.div, B, Fn, c.H, cus)
    return bool(dl.sum() * inv > 2 * kind_loss[1] or (dg > 2 * ln["bar_g"]).any())


def applies(c, X, cus, wrong):
    """None if the defect must leave a bar on this case, else why it cannot"""
    B, L, Fn, H = X["B"], c.L, c.F, c.H
    nw = nwg_of(B, cus)
    valid = X["y"] != PAD
    if wrong == "tail_lo_dropped" and Fn <= 128:
        return "no tail panel"
    if wrong == "half_chunk_dropped" and Fn % 8 != 4:
        return "no half chunk"
    if wrong == "rows128_dropped" and L <= 128:
        return "one row half"
    if wrong == "first_slate_only" and B <= nw:
        return "one slate per workgroup"
    if wrong == "reduce_g64" and nw <= 64:
        return "one trip of the reduce"
    if wrong == "relu_ge" and not c.act:
        return "no ReLU"
    if wrong == "pad_kept" and valid[valid.any(1)].all():
        return "no padded slot in a live slate"
    if wrong == "eps_outside" and not eps_shift_shows(c, X, cus):
        return "eps against P of ordinary size: what eps outside the log moves is within twice the bar of the loss and of every d loss / d score"
    if wrong == "label_no_max" and not (X["y"].max(1) > 89).any():
        return "no label whose exponential overflows"
    if wrong == "B_divisor" and c.div_mul == 1.0:
        return "batch_divisor is B"
    if wrong == "no_D_b1":
        return "D = sum dscore is 0 in exact arithmetic (sum P = 1 in every live slate): D b1 is a rounding residue inside the bar of dw_out on any input"
    if wrong in ("last_twice", "first_slate_only", "rows128_dropped", "reduce_g64", "no_xh_dhl") and not valid.sum(1).max() > 1:
        return "no slate with two valid items: every gradient is a rounding residue"
    return None


def wrongs(c):
    return FC_WRONG if c.kind == "fc" else LIN_WRONG
