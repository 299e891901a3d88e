"""fp64 references, a-priori entrywise bars, fp32 transcriptions and case tables of the loss kernels of allrank_amd/csrc/ltrx_pointpair.hip
--  TEST INFRASTRUCTURE, plain numpy, needs no GPU.  The layout of tests/listwise_ref.py (read its header first; U, gam, P_LIBM, FLT_MIN,
comp, k_block, Batch, _block_sum32, _strided32, _softmax_err, _finalize are its).  Four sections, each with its chain in its header:

    ltrx_ranknet_fwd_bwd           ranknet_ref / ranknet_bar / ranknet_f32, RANKNET_WRONG, CASES           (this header)
    ltrx_bce_fwd_bwd               bce_ref / bce_f32, BCE_WRONG, BCE_CASES: bce (n = 0) and ordinal (n = 1, 3, 4)
    ltrx_pointwise_rmse_fwd_bwd    rmse_ref / rmse_f32, RMSE_WRONG, RMSE_CASES
    ltrx_binary_listnet_fwd_bwd    blistnet_ref / blistnet_f32, BLISTNET_WRONG, BLISTNET_CASES

A reference returns its bars with it (bar_loss, bar_per, bar_grad); `checks` / `plain_checks` pair every output with them.  The two helpers
the count-normalised losses share: ltrx_ratio_finalize_kernel's strided loop is reached by the B = 257 cases of rankNet and bce, the second
grid-stride trip of ltrx_scale_by_device_kernel by the ordinal case B = 64, L = 2049, n = 4 alone.  rankNet:

    ranknet_ref   fp64 on the fp32 operands, one slate at a time in row chunks of CHUNK items (L = 2048 needs no L x L matrix): the loss,
                  the gradient, the pair count, the per-slate (sum, count) at the head of the workspace, and per entry the sum of |terms|
                  and the propagated error
    ranknet_bar   (fp32 roundings on the longest path) * u * (sum of |terms|) + propagated error.  No measured number.
    ranknet_f32   the kernel's arithmetic in np.float32 in source order (thread t owns items t, t + 256, ... and walks all L partners of
                  each), with ``wrong=`` one-line defects

The chain.  d = s_hi - s_lo (hi: the item with the larger label) moves the argument by u |d|; both orientations of a pair form the same d.
  sigmoid_neg(d) = 1 / (1 + expf(d)): E = e^d carries dE = expm1(u |d|)(1 + P u) + P u; 1 + E: dE E / (1 + E) = dE (1 - sn) and u; the
  division u: dsn = comp(dE (1 - sn), u, u) relatively, + FLT_MIN absolutely (expf overflows to inf at score scale 30 and sn is 0.f where
  the true value is below FLT_MIN).  softplus_neg(d) = fmaxf(-d, 0) + log1pf(expf(-|d|)): fmaxf is exact and carries the argument's u |d|;
  x = e^-|d| as E; log1pf has slope <= 1: x dE + FLT_MIN, and P u log1p(x); the addition u.  The weight: 1 (mode 0), |y_i - y_j| one
  rounding (mode 1), |y_i^2 - y_j^2| three (mode 2) -- all exact for integer labels, which `inputs` asserts; the bar still counts them.
  The product with the weight u.  A gradient entry is a thread's serial walk over the L partners: gam(L) on sum |w sn|.  per_sum: a
  thread's ceil(L / 256) items times L partners, then block_sum: k_block(ceil(L / 256) L, 256).  The finalize: k_block(ceil(B / 256), 256)
  on the per-slate sums; the counts are sums of 1.f below 2^24 (asserted): exact; sa / d one rounding; inv = 1 / d one; the in-place
  g *= inv one.

Exact, compared bit for bit: padded gradient entries 0.f; per_cnt, pair_count_out; a slate without pairs contributes (0, 0); a batch
without pairs gives a NaN loss and a gradient that is exactly 0.  `yi > yj`, `y != pad` involve no arithmetic.  No input is redrawn and no
entry is left out of any comparison."""
import functools
import os
import re
from collections import namedtuple

import numpy as np

from tests.listwise_ref import (CHUNK, PAD, Batch, F, FLT_MIN, ONE, P_LIBM, U, _block_sum32, _finalize, _finalize32, _softmax_err, _strided32, comp,  # noqa: F401
                                f64, gam, k_block, over, w, worst)

MAX_L = 2048


def workspace_bytes(B):
    return max(B, 0) * 2 * 4 + 64


def source_constants():
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "allrank_amd", "csrc")
    pp = open(os.path.join(here, "ltrx_pointpair.hip")).read()
    hdr = open(os.path.join(here, "..", "..", "include", "ltrx.h")).read()
    out = dict(max_l=int(re.search(r"#define LTRX_MAX_SLATE_LEN (\d+)", hdr).group(1)))
    out["ranknet_threads"] = re.findall(r"ltrx_ranknet_kernel, dim3\(B\), dim3\((\d+)\), 2 \* \(size_t\)L \* sizeof\(float\)", pp)
    out["finalize_threads"] = re.findall(r"ltrx_ratio_finalize_kernel, dim3\(1\), dim3\((\d+)\)", pp)
    m = re.search(r"size_t blocks = \(n_grad \+ 255\) / 256;\s+if \(blocks > (\d+)\) blocks = (\d+);", pp)
    out["scale_blocks"] = (int(m.group(1)), int(m.group(2)))
    assert re.search(r"ltrx_ranknet_workspace_bytes\(int B, int L\) \{\s+\(void\)L;\s+return \(size_t\)\(B > 0 \? B : 0\) \* 2 \* sizeof\(float\) \+ 64;", pp)
    return out


def _weight(mode, yh, yl):
    """(w, its relative rounding count) of the pairs hi x lo"""
    if mode == 0:
        return np.ones(np.broadcast(yh, yl).shape), 0
    if mode == 1:
        return np.abs(yh - yl), 1
    return np.abs(yh * yh - yl * yl), 3


def ranknet_ref(bt, mode, ext=None):
    B, L = bt.B, bt.L
    per, d_per, cnt, grads, bars = np.zeros(B), np.zeros(B), np.zeros(B), [], []
    k_g, k_l = L, k_block(-(-L // 256) * L, 256)
    for b, (s, y, valid) in enumerate(bt.slates()):
        g, A, E = np.zeros(L), np.zeros(L), np.zeros(L)
        idx = np.flatnonzero(valid)
        sv, yv = f64(s)[idx], f64(y)[idx]
        nv = len(idx)
        for lo in range(0, nv, CHUNK):
            I = slice(lo, min(nv, lo + CHUNK))
            sel = yv[I, None] > yv[None, :]                       # rows: the item with the larger label
            d = sv[I, None] - sv[None, :]
            wt, kw = _weight(mode, yv[I, None], yv[None, :])
            ad = np.abs(d)
            dE = np.expm1(U * ad) * (1 + P_LIBM * U) + P_LIBM * U
            e = np.exp(np.clip(d, -700.0, 700.0))
            sn = 1.0 / (1.0 + e)
            t = np.where(sel, wt * sn, 0.0)
            terr = np.where(sel, t * comp(gam(kw), comp(dE * (1.0 - sn), U, U), U) + wt * FLT_MIN * (1 + 4 * U), 0.0)
            x = np.exp(-ad)
            l1p = np.log1p(x)
            hinge = np.maximum(-d, 0.0)
            sp = hinge + l1p
            dsp = U * hinge + x * dE + FLT_MIN + P_LIBM * U * l1p
            dsp = dsp + U * (sp + dsp)
            lt = np.where(sel, wt * sp, 0.0)
            dlt = np.where(sel, wt * dsp + (lt + wt * dsp) * comp(gam(kw), U), 0.0)
            per[b] += lt.sum()
            d_per[b] += dlt.sum()
            cnt[b] += sel.sum()
            rows, cols = t.sum(1), t.sum(0)
            g[idx[I]] -= rows
            g[idx] += cols
            A[idx[I]] += rows
            A[idx] += cols
            E[idx[I]] += terr.sum(1)
            E[idx] += terr.sum(0)
        d_per[b] = d_per[b] + gam(k_l) * (per[b] + d_per[b])
        grads.append(g), bars.append(E + gam(k_g) * (A + E))
    assert cnt.sum() < 2 ** 24
    count = float(cnt.sum())
    den = count if ext is None else float(F(ext))
    kf = k_block(-(-B // 256), 256)
    sa = per.sum()
    e_sa = d_per.sum() + gam(kf) * (sa + d_per.sum())
    g, bg = np.stack(grads), np.stack(bars)
    with np.errstate(invalid="ignore", divide="ignore"):
        loss = sa / den if den != 0 else float("nan")
        bar_loss = (e_sa + U * (sa + e_sa)) / den if den > 0 else 0.0
        inv = 1.0 / den if den > 0 else 0.0
    return dict(loss=loss, per=per, per_count=cnt, count=count, grad=g * inv, bar_loss=bar_loss, bar_per=d_per,
                bar_grad=inv * (bg * (1 + gam(2)) + gam(2) * np.abs(g)), zero=(bt.y == PAD) | (den <= 0))


def ranknet_bar(ref):
    return dict(loss=ref["bar_loss"], per=ref["bar_per"], grad=ref["bar_grad"])


RANKNET_WRONG = ("tie_counted", "mode2_as_square_of_diff", "else_arm_sign", "both_orientations_counted", "tail_item_dropped",
                 "own_count_despite_ext", "softplus_without_max", "inv_applied_twice")
# not a gross defect: 1 - sigmoid(d) for sigmoid(-d) is off by an ABSOLUTE u, which only the saturated (light) pairs feel
RANKNET_SUBTLE = ("sigmoid_as_one_minus",)


def ranknet_f32(bt, mode, ext=None, wrong=None):
    B, L = bt.B, bt.L
    passes = -(-L // 256)
    W = passes * 256
    s, y = np.zeros((B, W), F), np.full((B, W), PAD, F)
    s[:, :L], y[:, :L] = bt.s, bt.y
    lsum, cnt = np.zeros((B, 256), F), np.zeros((B, 256), F)
    grad = np.zeros((B, W), F)
    last = (L // 256) if wrong == "tail_item_dropped" else passes
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        for m in range(last):
            I = slice(m * 256, (m + 1) * 256)
            si, yi = s[:, I], y[:, I]
            vi = yi != PAD
            g = np.zeros((B, 256), F)
            for j in range(L):
                sj, yj = s[:, j:j + 1], y[:, j:j + 1]
                live = vi & (yj != PAD) & ((yj != yi) | (wrong == "tie_counted"))
                if mode == 1:
                    wt = np.abs(yi - yj)
                elif mode == 2:
                    wt = ((yi - yj) * (yi - yj)) if wrong == "mode2_as_square_of_diff" else np.abs(yi * yi - yj * yj)
                else:
                    wt = np.ones_like(yi)
                hi = yi > yj
                d = np.where(hi, si - sj, sj - si).astype(F)
                if wrong == "softplus_without_max":
                    sp = np.log1p(np.exp(-d)).astype(F)
                else:
                    sp = (np.maximum(-d, F(0)) + np.log1p(np.exp(-np.abs(d)))).astype(F)
                if wrong == "sigmoid_as_one_minus":
                    sn = (ONE - (ONE / (ONE + np.exp(-d))).astype(F)).astype(F)
                else:
                    sn = (ONE / (ONE + np.exp(d))).astype(F)
                a = live & hi
                lsum = np.where(a, lsum + wt * sp, lsum).astype(F)
                cnt = np.where(a | (live & (wrong == "both_orientations_counted")), cnt + ONE, cnt).astype(F)
                down = a | (live & (wrong == "else_arm_sign"))
                g = np.where(live, np.where(down, g - wt * sn, g + wt * sn), g).astype(F)
            grad[:, I] = g
        per = np.array([_block_sum32(lsum[b]) for b in range(B)], F)
        pc = np.array([_block_sum32(cnt[b]) for b in range(B)], F)
        sa, sc = _block_sum32(_strided32(per, 256)), _block_sum32(_strided32(pc, 256))
        d = sc if (ext is None or wrong == "own_count_despite_ext") else F(ext)
        loss = F(sa / d)
        inv = F(ONE / d) if d > 0 else F(0)
        grad = (grad[:, :L] * inv).astype(F)
        if wrong == "inv_applied_twice":
            grad = (grad * inv).astype(F)
    return dict(loss=loss, per=per, per_count=pc, count=float(sc), grad=grad)


# ---------------------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name L scale mode ext B")
SHORT = (1, 2, 3, 4, 5, 255, 256, 257)
KILO = (1023, 1024, 1025, 2048)


def _cases():
    out = []

    def add(L, scale, mode, ext=None, B=5):
        out.append(Case("ranknet L %d scale %d mode %d%s%s" % (L, scale, mode, "" if ext is None else " ext count", "" if B == 5 else " B %d" % B),
                        L, scale, mode, ext, B))

    for L in SHORT:
        for scale in (1, 30):
            for mode in (0, 1, 2):
                add(L, scale, mode)
    for L in (5, 257):
        add(L, 1, 2, ext=977.0)
    for L in KILO:
        add(L, 30, 2)
        add(L, 1, 0)
    add(3, 1, 1, B=257)                                            # the finalize's strided loop: thread 0 adds slate 0 and slate 256
    return out


CASES = _cases()


@functools.lru_cache(maxsize=None)
def _inputs(L, scale, B):
    rng = np.random.default_rng([L, scale, B])
    s = rng.standard_normal((B, L))
    y = rng.integers(0, 5, (B, L)).astype(np.float64)
    counts = (L, 1, 0, max(1, L // 2), L) if B == 5 else tuple(rng.integers(0, L + 1, B))
    for b, nv in enumerate(counts):
        if b == 3:
            s[b] = np.round(s[b] * 10) / 10                        # tie-heavy
        elif nv >= 2:
            s[b, nv - 1] = s[b, 0]
        if b == 4:
            y[b] = 3                                               # equal labels: no pair
        y[b, nv:] = float(PAD)
    bt = Batch((s.astype(F) * F(scale)).astype(F), y.astype(F))
    assert np.array_equal(bt.y, np.round(bt.y)) and np.abs(bt.y).max() <= 4, "integer labels: the weights are exact"
    bt.s.setflags(write=False), bt.y.setflags(write=False)
    return bt


def inputs(c):
    """scores N(0, 1) x scale in fp32 with exact ties, integer labels 0..4.  B = 5: a full slate, one padded to 1 valid item, an all-padded
    one, a half-padded tie-heavy one (scores rounded to 0.1) and a full one of equal labels.  The B = 257 case is about the finalize's
    strided loop alone: every slate draws its own number of valid items, so slates 3 (tie-heavy) and 4 (equal labels) are of arbitrary
    length there.  ext_pair_count is given in mode 2 at L = 5 and 257 only: the finalize that reads it does not see the mode."""
    return _inputs(c.L, c.scale, c.B)


@functools.lru_cache(maxsize=None)
def reference(c):
    return ranknet_ref(inputs(c), c.mode, c.ext)


def transcription(c, wrong=None):
    return ranknet_f32(inputs(c), c.mode, c.ext, wrong)


def checks(c, got, ref=None):
    ref = reference(c) if ref is None else ref
    out = dict(per=(got["per"], ref["per"], ref["bar_per"]))
    if "grad" in got:
        out["grad"] = (got["grad"], ref["grad"], ref["bar_grad"])
    if not np.isnan(ref["loss"]):
        out["loss"] = (got["loss"], ref["loss"], ref["bar_loss"])
    return out


def exact_ok(c, got, ref=None):
    ref = reference(c) if ref is None else ref
    ok = np.array_equal(np.asarray(got["per_count"], np.float64), ref["per_count"]) and (got.get("count", ref["count"]) == ref["count"])
    ok = ok and not np.asarray(got["per"])[ref["per_count"] == 0].any()
    if "grad" in got:
        ok = ok and not np.asarray(got["grad"])[ref["zero"]].any()
    if np.isnan(ref["loss"]):
        ok = ok and bool(np.isnan(got["loss"]))
    return bool(ok)


def applies(c, wrong):
    if c.L < 2:
        return "one item has no partner"
    if wrong == "tie_counted" and c.mode != 0:
        return "a tie has weight 0 in modes 1 and 2"
    if wrong == "mode2_as_square_of_diff" and c.mode != 2:
        return "mode 2 only"
    if wrong == "tail_item_dropped" and c.L % 256 == 0:
        return "no tail"
    if wrong == "own_count_despite_ext" and c.ext is None:
        return "ext_pair_count is NULL"
    if wrong == "softplus_without_max" and c.scale == 1:
        return "expf does not overflow at N(0, 1) scores"
    return None


# ---------------------------------------------------------------------------------------------------------------------------------
# bce (n = 0) and ordinal (n >= 1): ltrx_bce_fwd_bwd
#
# The chain.  p is an operand.  logf(p): P u |log p|.  q = fl(1 - p) is off by u q (exact for p >= 0.5), which moves log q by u / (1 - u);
#   logf(q): P u |log q|.  max(., -100) is 1-Lipschitz and log 0 = -inf clamps to -100.f exactly on both sides.  t and 1 - t are small
#   integers: exact.  The two products and their sum: gam(3) on |t lp| + |(1 - t) lq|.  A thread adds ceil(L nn / 256) summands, then
#   block_sum: k_block(ceil(L nn / 256), 256).  g = (p - t) / max((1 - p) p, 1e-12f): the subtraction u, the denominator gam(2) (max is
#   1-Lipschitz and the clamp only enlarges it), the division u.  The counts are exact.  The finalize and the in-place g *= inv as for rankNet;
#   ltrx_scale_by_device_kernel runs 2048 blocks of 256 threads at most, so a gradient of more than 524288 entries takes its second trip.
# ---------------------------------------------------------------------------------------------------------------------------------
BCE_CLAMP = float(F(1e-12))
SCALE_GRID = 2048 * 256


def _finalize_ratio(per, d_per, cnt, ext):
    """(loss, bar_loss, inv, den) of ltrx_ratio_finalize_kernel"""
    B = len(per)
    assert cnt.sum() < 2 ** 24
    den = float(cnt.sum()) if ext is None else float(F(ext))
    kf = k_block(-(-B // 256), 256)
    sa, ab = per.sum(), np.abs(per).sum()
    e_sa = d_per.sum() + gam(kf) * (ab + d_per.sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        loss = sa / den if den != 0 else float("nan")
        bar = (e_sa + U * (abs(sa) + e_sa)) / den if den > 0 else 0.0
        inv = 1.0 / den if den > 0 else 0.0
    return loss, bar, inv, den


def bce_ref(y, p, n, ext=None):
    """y [B, L] labels, p [B, L] (n = 0) or [B, L, n] probabilities, all fp32"""
    B, L = y.shape
    nn = max(n, 1)
    p, yv = f64(p).reshape(B, L, nn), f64(y)
    valid = (yv != float(PAD))[:, :, None]
    t = (yv[:, :, None] >= np.arange(1, nn + 1)[None, None, :]).astype(np.float64) if n > 0 else yv[:, :, None]
    q = 1.0 - p
    with np.errstate(divide="ignore"):
        lp, lq = np.maximum(np.log(p), -100.0), np.maximum(np.log(q), -100.0)
    dlp = np.where(p == 0, 0.0, P_LIBM * U * np.abs(lp))
    dlq = np.where(q == 0, 0.0, U / (1 - U) + P_LIBM * U * np.abs(lq))
    a, b = t * lp, (1.0 - t) * lq
    ab = np.abs(a) + np.abs(b)
    err = np.abs(t) * dlp + np.abs(1.0 - t) * dlq
    err = err + gam(3) * (ab + err)
    term, ab, err = np.where(valid, -(a + b), 0.0), np.where(valid, ab, 0.0), np.where(valid, err, 0.0)
    k = k_block(-(-L * nn // 256), 256)
    per = term.sum((1, 2))
    d_per = err.sum((1, 2)) + gam(k) * (ab.sum((1, 2)) + err.sum((1, 2)))
    nvalid = valid[:, :, 0].sum(1).astype(np.float64)
    cnt = nvalid if n > 0 else (nvalid > 0).astype(np.float64)
    g = np.where(valid, (p - t) / np.maximum(q * p, BCE_CLAMP), 0.0)
    bg = np.abs(g) * comp(U, (1.0 + 0.0) / (1.0 - gam(2)) - 1.0, U)
    loss, bar_loss, inv, den = _finalize_ratio(per, d_per, cnt, ext)
    shape = (B, L, nn) if n > 0 else (B, L)
    return dict(loss=loss, per=per, per_count=cnt, count=float(cnt.sum()), grad=(g * inv).reshape(shape), bar_loss=bar_loss, bar_per=d_per,
                bar_grad=(inv * (bg * (1 + gam(2)) + gam(2) * np.abs(g))).reshape(shape),
                zero=np.broadcast_to(~valid | (den <= 0), (B, L, nn)).reshape(shape))


BCE_WRONG = ("bce_counts_items", "ordinal_counts_slates", "target_gt_instead_of_ge", "k_off_by_one", "layout_BnL", "log_clamp_dropped",
             "denominator_clamp_dropped")


def bce_f32(y, p, n, ext=None, wrong=None):
    B, L = y.shape
    nn = max(n, 1)
    p = np.asarray(p, F).reshape(B, L, nn)
    if wrong == "layout_BnL":
        p = p.reshape(B, nn, L).transpose(0, 2, 1)
    y3 = np.asarray(y, F)[:, :, None]
    valid = np.broadcast_to(y3 != PAD, (B, L, nn))
    ks = np.arange(0 if wrong == "k_off_by_one" else 1, nn + (0 if wrong == "k_off_by_one" else 1)).astype(F)[None, None, :]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if n > 0:
            t = ((y3 > ks) if wrong == "target_gt_instead_of_ge" else (y3 >= ks)).astype(F)
        else:
            t = np.broadcast_to(y3, (B, L, nn)).astype(F)
        q = (ONE - p).astype(F)
        lp, lq = np.log(p).astype(F), np.log(q).astype(F)
        if wrong != "log_clamp_dropped":
            lp, lq = np.maximum(lp, F(-100)), np.maximum(lq, F(-100))
        term = np.where(valid, -((t * lp).astype(F) + ((ONE - t) * lq).astype(F)), F(0)).astype(F)
        den = (q * p).astype(F) if wrong == "denominator_clamp_dropped" else np.maximum((q * p).astype(F), F(1e-12))
        g = np.where(valid, (p - t).astype(F) / den, F(0)).astype(F)
        per = np.array([_block_sum32(_strided32(term[b].ravel(), 256)) for b in range(B)], F)
        nv = np.array([_block_sum32(_strided32(valid[b, :, 0].astype(F), 256)) for b in range(B)], F)
        items = (n > 0 and wrong != "ordinal_counts_slates") or (n == 0 and wrong == "bce_counts_items")
        pc = nv if items else (nv > 0).astype(F)
        sa, sc = _block_sum32(_strided32(per, 256)), _block_sum32(_strided32(pc, 256))
        d = sc if ext is None else F(ext)
        loss = F(sa / d)
        inv = F(ONE / d) if d > 0 else F(0)
        g = (g * inv).astype(F)
    return dict(loss=loss, per=per, per_count=pc, count=float(sc), grad=g.reshape((B, L, nn) if n > 0 else (B, L)))


BCase = namedtuple("BCase", "name L n ext B")
BCE_L = SHORT + KILO + (2049,)


def _bce_cases():
    out = []

    def add(L, n, ext=None, B=5):
        out.append(BCase("%s L %d%s%s%s" % ("ordinal" if n else "bce", L, " n %d" % n if n else "", "" if ext is None else " ext count",
                                            "" if B == 5 else " B %d" % B), L, n, ext, B))

    for L in BCE_L:
        add(L, 0)
        for n in (1, 3, 4):
            if L in (1, 5, 257, 2049) or n == 3:
                add(L, n)
    add(5000, 0)
    add(5, 0, ext=13.0), add(257, 3, ext=977.0)
    add(3, 0, B=257)                                               # the finalize's strided loop
    add(2049, 4, B=64)                                             # 524544 gradient entries: the second trip of ltrx_scale_by_device_kernel
    return out


BCE_CASES = _bce_cases()
SPECIAL_P = (0.0, 1.0, 2.0 ** -24, 1.0 - 2.0 ** -24)


@functools.lru_cache(maxsize=None)
def bce_inputs(c):
    """(y [B, L], p): labels 0 / 1 for bce and 0..4 for ordinal, probabilities uniform in (0.02, 0.98) with exactly 0, exactly 1, 2^-24
    and 1 - 2^-24 on the first items of the full slates; a full slate, one padded to 1 valid item, an all-padded one, a half-padded one and
    a full one of equal labels (B = 5), or random valid counts"""
    rng = np.random.default_rng([c.L, c.n, c.B])
    B, L, nn = c.B, c.L, max(c.n, 1)
    y = rng.integers(0, 5 if c.n else 2, (B, L)).astype(np.float64)
    counts = (L, 1, 0, max(1, L // 2), L) if B == 5 else tuple(rng.integers(0, L + 1, B))
    for b, nv in enumerate(counts):
        if b == 4 and B == 5:
            y[b] = 1
        y[b, nv:] = float(PAD)
    p = rng.uniform(0.02, 0.98, (B, L, nn)).astype(F)
    flat = p.reshape(B, -1)
    for b in (0, 4 % B):
        for i, v in enumerate(SPECIAL_P[:flat.shape[1]]):
            flat[b, (i + b) % flat.shape[1]] = F(v)
    assert B * L < 2 ** 24
    y, p = y.astype(F), (p if c.n else p[:, :, 0]).copy()
    y.setflags(write=False), p.setflags(write=False)
    return y, p


@functools.lru_cache(maxsize=None)
def bce_reference(c):
    y, p = bce_inputs(c)
    return bce_ref(y, p, c.n, c.ext)


def bce_transcription(c, wrong=None):
    y, p = bce_inputs(c)
    return bce_f32(y, p, c.n, c.ext, wrong)


def bce_applies(c, wrong):
    if wrong == "bce_counts_items" and (c.n or c.L < 2):
        return "ordinal, or one item per slate"
    if wrong in ("ordinal_counts_slates", "target_gt_instead_of_ge", "k_off_by_one") and (not c.n or (c.L < 2 and wrong == "ordinal_counts_slates")):
        return "bce, or one item per slate"
    if wrong == "layout_BnL" and (c.n < 2 or c.L < 2):
        return "one output per item"
    return None


# ---------------------------------------------------------------------------------------------------------------------------------
# pointwise_rmse: ltrx_pointwise_rmse_fwd_bwd
#
# The chain.  e = y - levels p: the product u |levels p|, the subtraction u |e| -- e cancels, so the bar is on |y| + |levels p|: gam(2) of
#   it (a fused multiply-add only removes a rounding).  e e: 2 |e| de + de^2 and the product u.  sq: k_block(ceil(L / 256), 256) on
#   positive terms; cnt is a sum of 1.f: exact.  sq / cnt u; sqrtf is correctly rounded and halves the relative error before it:
#   rho / (2 (1 - rho)), and u.  The gradient -levels e / (cnt rmse) inv_div: the product with levels u on top of levels de; cnt rmse u;
#   the division, inv_div = 1 / divisor and the product with it gam(3).  The loss is ltrx_launch_finalize_sum (tests/listwise_ref.py:
#   _finalize).  Exact: padded entries 0.f; a slate fitted exactly (every levels p == y in fp32, asserted by `rmse_inputs`) has rmse 0.f
#   and the gradient 0 / 0 = NaN on its valid items, as the kernel's comment states and torch's sqrt' gives; an all-padded slate has
#   cnt = 0, rmse = 0 / 0 = NaN, and with it the loss is NaN.
# ---------------------------------------------------------------------------------------------------------------------------------
def rmse_ref(y, p, levels, batch_divisor):
    B, L = y.shape
    lv, inv = w(levels), 1.0 / w(batch_divisor)
    k = k_block(-(-L // 256), 256)
    per, d_per = np.zeros(B), np.zeros(B)
    g, bg = np.zeros((B, L)), np.zeros((B, L))
    nan_grad = np.zeros((B, L), bool)
    for b in range(B):
        valid = y[b] != PAD
        nv = int(valid.sum())
        if nv == 0:
            per[b] = np.nan
            continue
        yv, lp = f64(y[b])[valid], lv * f64(p[b])[valid]
        e = yv - lp
        if not e.any():
            assert np.array_equal((F(levels) * p[b][valid]).astype(F), y[b][valid]), "an exactly fitted slate must be exact in fp32 too"
            nan_grad[b] = valid
            continue
        de = gam(2) * (np.abs(yv) + np.abs(lp))
        e2 = e * e
        de2 = 2 * np.abs(e) * de + de * de
        de2 = de2 + U * (e2 + de2)
        sq = e2.sum()
        dsq = de2.sum() + gam(k) * (sq + de2.sum())
        rho = dsq / sq
        assert rho < 0.25, "sq has no relative precision"
        rq = comp(rho, U)
        rr = comp(rq / (2 * (1 - rq)), U)
        rmse = np.sqrt(sq / nv)
        per[b], d_per[b] = rmse, rmse * rr
        num = lv * e
        dnum = lv * de + U * (np.abs(num) + lv * de)
        den, dden = nv * rmse, comp(rr, U)
        g[b, valid] = -num / den * inv
        bg[b, valid] = inv / den * ((np.abs(num) + dnum) * (1 + gam(3)) / (1 - dden) - np.abs(num))
    nan_per = np.isnan(per)
    if nan_per.any():
        loss, bar_loss = float("nan"), 0.0
    else:
        tot, bar_loss = _finalize(per, d_per, inv)
        loss = tot * inv
    return dict(loss=loss, per=per, grad=g, bar_loss=bar_loss, bar_per=d_per, bar_grad=bg, zero=y == PAD, nan_grad=nan_grad, nan_per=nan_per)


RMSE_WRONG = ("divides_by_L", "levels_dropped_in_grad", "inv_div_twice", "padded_counted")


def rmse_f32(y, p, levels, batch_divisor, wrong=None):
    B, L = y.shape
    lv, inv = F(levels), F(ONE / F(batch_divisor))
    per, g = np.zeros(B, F), np.zeros((B, L), F)
    with np.errstate(invalid="ignore", divide="ignore"):
        for b in range(B):
            valid = y[b] != PAD
            use = np.ones(L, bool) if wrong == "padded_counted" else valid
            e = (y[b] - (lv * p[b]).astype(F)).astype(F)
            sq = _block_sum32(_strided32(np.where(use, (e * e).astype(F), F(0)).astype(F), 256))
            cnt = F(L) if wrong == "divides_by_L" else _block_sum32(_strided32(use.astype(F), 256))
            rmse = np.sqrt(F(sq / cnt)).astype(F)
            per[b] = rmse
            num = (-e if wrong == "levels_dropped_in_grad" else (-lv * e)).astype(F)
            gb = ((num / F(cnt * rmse)).astype(F) * inv).astype(F)
            if wrong == "inv_div_twice":
                gb = (gb * inv).astype(F)
            g[b] = np.where(valid, gb, F(0))
        loss = _finalize32(per, inv)
    return dict(loss=loss, per=per, grad=g)


RCase = namedtuple("RCase", "name L levels allpad")
RMSE_L = SHORT + KILO + (2049, 5000)
RMSE_CASES = [RCase("pointwise_rmse L %d levels %d" % (L, lv), L, lv, False) for L in RMSE_L for lv in (1, 4)] + [
    RCase("pointwise_rmse L 5 levels 4 with an all-padded slate", 5, 4, True)]


@functools.lru_cache(maxsize=None)
def rmse_inputs(c):
    """(y [B, L], p): labels 0..4, predictions uniform in (0, 1); a full slate, one padded to 1 valid item, a half-padded one fitted to
    about 1e-3 and a full one fitted exactly (levels p == y in fp32); `allpad` adds an all-padded slate"""
    rng = np.random.default_rng([c.L, c.levels, int(c.allpad)])
    L = c.L
    counts = (L, 1, max(1, L // 2), L) + ((0,) if c.allpad else ())
    B = len(counts)
    y = rng.integers(0, 5, (B, L)).astype(np.float64)
    p = rng.uniform(0.0, 1.0, (B, L))
    p[2] = (y[2] + 1e-3 * rng.standard_normal(L)) / c.levels
    p[3] = y[3] / c.levels
    for b, nv in enumerate(counts):
        y[b, nv:] = float(PAD)
    y, p = y.astype(F), p.astype(F)
    assert np.array_equal((F(c.levels) * p[3]).astype(F), y[3]) and B * L < 2 ** 24
    y.setflags(write=False), p.setflags(write=False)
    return y, p


@functools.lru_cache(maxsize=None)
def rmse_reference(c):
    y, p = rmse_inputs(c)
    return rmse_ref(y, p, c.levels, float(len(y)))


def rmse_transcription(c, wrong=None):
    y, p = rmse_inputs(c)
    return rmse_f32(y, p, c.levels, float(len(y)), wrong)


def rmse_applies(c, wrong):
    if wrong in ("divides_by_L", "padded_counted") and c.L < 2:
        return "no padded item"
    if wrong == "levels_dropped_in_grad" and c.levels == 1:
        return "levels 1"
    return None


# ---------------------------------------------------------------------------------------------------------------------------------
# binary_listNet: ltrx_binary_listnet_fwd_bwd.  ListNet (tests/listwise_ref.py: listnet_ref, whose chain and P -- _softmax_err -- are
#   reused) with the target T_i = y_i / norm, norm = sum of the valid labels (a sum of small integers: exact) or 1 when that is 0 (`ysum ==
#   0` involves no arithmetic): one division, dT = u T.  `T != 0` is exact.  A slate of zero labels has T = 0, rsum = 0: loss 0 and
#   a gradient of exactly 0; an all-padded slate likewise.
# ---------------------------------------------------------------------------------------------------------------------------------
EPS = 1e-10


def blistnet_ref(bt, eps, batch_divisor):
    eps, inv = w(eps), 1.0 / w(batch_divisor)
    per, d_per, grads, bars = [], [], [], []
    for s, y, valid in bt.slates():
        n = len(s)
        P, dP = _softmax_err(s, valid, 256)
        ysum = f64(y)[valid].sum()
        T = np.where(valid, f64(y), 0.0) / (ysum if ysum != 0 else 1.0)
        dT = U * T
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
    z = np.zeros(bt.s.shape, bool)
    return dict(loss=tot * inv, per=per, grad=np.stack(grads), bar_loss=d_loss, bar_per=d_per * (1 + U), bar_grad=np.stack(bars), zero=bt.y == PAD,
                nan_grad=z, nan_per=np.zeros(bt.B, bool))


BLISTNET_WRONG = ("norm_unguarded", "eps_dropped_in_r", "padded_in_softmax", "inv_div_twice")


def blistnet_f32(bt, eps, batch_divisor, wrong=None):
    eps, inv = F(eps), F(ONE / F(batch_divisor))
    per, grads = [], []
    for s, y, valid in bt.slates():
        with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
            x = s.astype(F) if wrong == "padded_in_softmax" else np.where(valid, s, -np.inf).astype(F)
            t = np.where(valid, y, F(0)).astype(F)
            smax = x.max()
            ysum = _block_sum32(_strided32(t, 256))
            e = np.where(x == -np.inf, F(0), np.exp((x - smax).astype(F))).astype(F)
            ssum = _block_sum32(_strided32(e, 256))
            inv_s = ONE / ssum if ssum > 0 else F(0)
            norm = ysum if (ysum != 0 or wrong == "norm_unguarded") else ONE
            P, T = (e * inv_s).astype(F), (t / norm).astype(F)
            lt = np.where(T != 0, T * np.log(P + eps), F(0)).astype(F)
            rt = (T * (P / (P + eps))).astype(F)
            lsum, rsum = _block_sum32(_strided32(lt, 256)), _block_sum32(_strided32(rt, 256))
            r = np.where(P > 0, P / (P if wrong == "eps_dropped_in_r" else (P + eps)), F(0)).astype(F)
            g = ((P * rsum - T * r) * inv).astype(F)
            if wrong == "inv_div_twice":
                g = (g * inv).astype(F)
        per.append(F(-lsum)), grads.append(g)
    return dict(loss=_finalize32(per, inv), per=np.array(per, F), grad=np.stack(grads))


LCase = namedtuple("LCase", "name L scale")
BLISTNET_CASES = [LCase("binary_listNet L %d scale %d" % (L, sc), L, sc) for L in SHORT for sc in (1, 30)] + [
    LCase("binary_listNet L %d scale 30" % L, L, 30) for L in KILO] + [LCase("binary_listNet L 2048 scale 1", 2048, 1)]


@functools.lru_cache(maxsize=None)
def blistnet_inputs(c):
    """scores N(0, 1) x scale in fp32 with exact ties, labels 0..4: a full slate, one padded to 1 valid item, an all-padded one, a
    half-padded tie-heavy one and a full one of zero labels (ysum == 0); padded slots hold scores of their own"""
    rng = np.random.default_rng([c.L, c.scale, 77])
    L = c.L
    s = rng.standard_normal((5, L))
    y = rng.integers(0, 5, (5, L)).astype(np.float64)
    for b, nv in enumerate((L, 1, 0, max(1, L // 2), L)):
        if b == 3:
            s[b] = np.round(s[b] * 10) / 10
        elif nv >= 2:
            s[b, nv - 1] = s[b, 0]
        if b == 4:
            y[b] = 0
        y[b, nv:] = float(PAD)
    bt = Batch((s.astype(F) * F(c.scale)).astype(F), y.astype(F))
    bt.s.setflags(write=False), bt.y.setflags(write=False)
    return bt


@functools.lru_cache(maxsize=None)
def blistnet_reference(c):
    bt = blistnet_inputs(c)
    return blistnet_ref(bt, EPS, float(bt.B))


def blistnet_transcription(c, wrong=None):
    bt = blistnet_inputs(c)
    return blistnet_f32(bt, EPS, float(bt.B), wrong)


def blistnet_applies(c, wrong):
    if wrong == "eps_dropped_in_r" and c.scale == 1:
        return "no P small enough against eps at N(0, 1) scores"
    if wrong == "padded_in_softmax" and c.L < 2:
        return "no slate with a valid and a padded item"
    return None


def plain_checks(got, ref):
    """{output: (got, ref, bar)} of pointwise_rmse and binary_listNet, over every entry whose reference is a number"""
    fin = ~ref["nan_per"]
    out = dict(per=(np.asarray(got["per"])[fin], ref["per"][fin], ref["bar_per"][fin]))
    if "grad" in got:
        keep = ~ref["nan_grad"]
        out["grad"] = (np.asarray(got["grad"])[keep], ref["grad"][keep], ref["bar_grad"][keep])
    if not np.isnan(ref["loss"]):
        out["loss"] = (got["loss"], ref["loss"], ref["bar_loss"])
    return out


def plain_exact_ok(got, ref):
    """padded zeros; the NaN gradient and the 0 rmse of an exactly fitted slate; the NaN rmse of an all-padded slate and the NaN loss"""
    ok = bool(np.isnan(np.asarray(got["per"])[ref["nan_per"]]).all()) and bool(np.isnan(got["loss"])) == bool(np.isnan(ref["loss"]))
    fitted = ref["nan_grad"].any(1)
    ok = ok and not np.asarray(got["per"])[fitted].any()
    if "grad" in got:
        g = np.asarray(got["grad"])
        ok = ok and not g[ref["zero"]].any() and bool(np.isnan(g[ref["nan_grad"]]).all())
    return bool(ok)
