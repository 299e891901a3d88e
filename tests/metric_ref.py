"""fp64 references, a-priori entrywise bars, fp32 transcriptions and the case table of the metric kernels: ltrx_ndcg_at, ltrx_ndcg_at_gains,
ltrx_ndcg_at_cu (allrank_amd/csrc/ltrx_ndcg.hip) and ltrx_mrr_at, ltrx_mrr_at_cu (allrank_amd/csrc/ltrx_pointpair.hip) --  TEST
INFRASTRUCTURE, plain numpy, needs no GPU.  The layout of tests/listwise_ref.py (read its header first; U, gam, P_LIBM, comp, k_scan, Batch,
_scan32, _gain are its):

    *_ref   the metric in fp64 on the fp32 operands as the kernel receives them, one slate at a time; every output (ndcg, dcg, order_out;
            mrr and the per-slate (best_val, best_idx) at the head of the workspace) and, per entry, the sum of |terms| and the propagated
            error.  tests/test_metric_ref_cpu.py holds it to oracle/ltr_oracle.py (dtype=np.float64) on the padded grid.
    *_bar   (fp32 roundings on the longest path) * u * (sum of |terms|) + propagated error.  No measured number.
    *_f32   the kernel's arithmetic in np.float32 in source order, with ``wrong=`` one-line defects.

Order and ranks.  The counting ranks, order_out and MRR's (best_val, best_idx) involve no arithmetic: exact, compared bit for bit.  The
  stable descending order comes from np.argsort(kind="stable") on the negated key (oracle.ltr_oracle.stable_argsort_desc), not from an L x L
  compare.  order_out is compared over the whole slate: the valid items in predicted order, then the padded items in index order; in the
  cu layout the indices are inside the slate.

NDCG.  gain = exp2f(y) - 1: P u 2^y + u gain absolutely, and exp2f(0) = 1 exactly, so a label 0 has gain 0 exactly (the assumption of
  tests/listwise_ref.py); a caller's gain (ltrx_ndcg_at_gains) is an operand: exact.  (float)rank + 2 is exact below 2^24; log2f P u; the
  division 1:  term_p = gain / log2f(p + 2) carries comp(dgain / gain, P u, u) relatively.  block_inclusive_scan over the slate's n
  items with the launcher's T threads: k_scan(n, T) roundings on sum_{p' <= p} |term_p'|, plus the terms' own errors.  The padded call
  scans n = L items (the padded tail holds 0.f, or the padded items' gains at their tail positions in the gains form) with T = 1024 above L
  = 512, else 256; the ragged call scans the slate's own length with T = 1024 above max_len = 256, else 256.  at = min(at, n); ndcg =
  d / id: (bar_d + |d / id| bar_id) / (|id| - bar_id) and u.  `id == 0` is exact for non-negative gains (a sum of non-negative terms is
  0.f only if every term is): the filler is compared bit for bit; for the one signed-gains case `inputs` asserts |id| > 2^10 bar_id at
  every cut-off.  Exact as well: an all-padded slate and a ragged slate of length 0 give (filler, 0).

MRR.  ymax, the ranks and the index are exact; tot = sum_b best_val[b] is a sum of integers 0..4 (exact), so `tot == 0` is; every entry
  is 0 or 1 / (idx + 1) correctly rounded.  The whole output is compared bit for bit against the fp32 transcription and to the fp64
  reference within u |value|.  mrr_ref and mrr_f32 share the exact part (_mrr_slates, _mrr_out) and differ in the dtype of the one
  division only, so the bit comparison says no more than "correctly rounded"; what holds the shared part is the oracle comparison of
  tests/test_metric_ref_cpu.py (every case up to L = 513 but the repeating order, the "zero batch" case included) and the defect models.
  A slate that a repeating slate_order never names: ltrx_mrr_at_cu clears (best_val, best_idx) to (0, 0) before the slate kernel runs,
  so such a slate counts as an empty one in the batch sum and its output row is 1 / 1 or 0 like an empty slate's (ltrx_ndcg_at_cu
  writes nothing for it: its rows keep what they held).  The GPU test fills the workspace with NaN first; the defect model
  "unvisited_not_cleared" is the kernel before the clear existed: the batch sum is NaN.

Thread counts and opt-ins (EXPECTED_ARMS, held to the source text by source_constants): ndcg asks for 4 * L * 4 bytes of dynamic LDS and opts
in above 48 KB (L > 3072), mrr for 2 * L * 4 bytes (L > 6144); mrr always launches 256 threads.
"""
import functools
import os
import re
from collections import namedtuple

import numpy as np

from tests.listwise_ref import (PAD, Batch, F, ONE, P_LIBM, U, _gain, _scan32, comp, f64, gam, k_scan, over, worst)  # noqa: F401

FILLER = F(0.25)                     # not 1: a wrongly taken filler branch cannot coincide with a perfect ranking
MAX_ATS = 16
MAX_METRIC_L = 8192
DEFAULT_DYN_LDS = 48 * 1024
RAGGED_LENGTHS = (0, 1, 2, 3, 5, 31, 32, 33, 64, 100, 255, 256, 257)       # tests/ragged_cases.py
NDCG_ENTRIES = ("ltrx_ndcg_at", "ltrx_ndcg_at_gains", "ltrx_ndcg_at_cu")
MRR_ENTRIES = ("ltrx_mrr_at", "ltrx_mrr_at_cu")


def threads(entry, L):
    """the launcher's workgroup size; L is max_len for the _cu entries"""
    if entry in MRR_ENTRIES:
        return 256
    return 1024 if L > (256 if entry.endswith("_cu") else 512) else 256


def lds_bytes(entry, L):
    return (2 if entry in MRR_ENTRIES else 4) * L * 4


def opts_in(entry, L):
    return lds_bytes(entry, L) > DEFAULT_DYN_LDS


def mrr_workspace_bytes(B):
    return max(B, 0) * 8 + 64


# (entry, L) -> (threads, opts in): the literal table of the lengths on either side of every switch
EXPECTED_ARMS = {
    ("ltrx_ndcg_at", 512): (256, False), ("ltrx_ndcg_at", 513): (1024, False), ("ltrx_ndcg_at", 3072): (1024, False),
    ("ltrx_ndcg_at", 3073): (1024, True), ("ltrx_ndcg_at", 8192): (1024, True),
    ("ltrx_ndcg_at_gains", 257): (256, False), ("ltrx_ndcg_at_gains", 3072): (1024, False),
    ("ltrx_ndcg_at_cu", 256): (256, False), ("ltrx_ndcg_at_cu", 257): (1024, False), ("ltrx_ndcg_at_cu", 3073): (1024, True),
    ("ltrx_mrr_at", 512): (256, False), ("ltrx_mrr_at", 513): (256, False), ("ltrx_mrr_at", 6144): (256, False),
    ("ltrx_mrr_at", 6145): (256, True), ("ltrx_mrr_at", 8192): (256, True),
    ("ltrx_mrr_at_cu", 256): (256, False), ("ltrx_mrr_at_cu", 257): (256, False), ("ltrx_mrr_at_cu", 3073): (256, False),
}


def source_constants():
    """the same numbers read from the source text"""
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "allrank_amd", "csrc")
    rd = lambda f: open(os.path.join(here, f)).read()     # noqa: E731
    nd, pp, dev = rd("ltrx_ndcg.hip"), rd("ltrx_pointpair.hip"), rd("ltrx_device.h")
    hdr = open(os.path.join(here, "..", "..", "include", "ltrx.h")).read()
    m = re.search(r"const dim3 block\(L > \(cu \? (\d+) : (\d+)\) \? (\d+) : (\d+)\);", nd)
    out = dict(ndcg_block=tuple(int(v) for v in m.groups()))
    assert re.search(r"if \(4 \* \(size_t\)L \* sizeof\(float\) > LTRX_DEFAULT_DYNAMIC_LDS_BYTES\) \{\s+static std::atomic<uint64_t> attr_done\{0\};"
                     r"\s+const int arc = ltrx_allow_dynamic_lds\(attr_done, \{\{ltrx_ndcg_kernel<false>", nd)
    assert re.search(r"if \(2 \* \(size_t\)L \* sizeof\(float\) > LTRX_DEFAULT_DYNAMIC_LDS_BYTES\) \{\s+static std::atomic<uint64_t> attr_done\{0\};"
                     r"\s+const int arc = ltrx_allow_dynamic_lds\(attr_done, \{\{ltrx_mrr_slate_kernel<false>", pp)
    out["ndcg_lds"] = sorted(set(re.findall(r"dim3\(B\), block, (\d+) \* \(size_t\)L \* sizeof\(float\)", nd)))
    out["mrr_launch"] = re.findall(r"ltrx_mrr_slate_kernel<(?:true|false)>, dim3\(B\), dim3\((\d+)\), (\d+) \* \(size_t\)L \* sizeof\(float\)", pp)
    out["default_lds"] = int(re.search(r"#define LTRX_DEFAULT_DYNAMIC_LDS_BYTES \((\d+) \* 1024\)", dev).group(1)) * 1024
    out["max_ats"] = int(re.search(r"#define LTRX_MAX_ATS (\d+)", dev).group(1))
    out["max_metric_l"] = int(re.search(r"#define LTRX_MAX_METRIC_SLATE_LEN (\d+)", hdr).group(1))
    assert re.search(r"ltrx_mrr_workspace_bytes\(int B, int L, int n_ats\) \{\s+\(void\)L;\s+\(void\)n_ats;\s+return \(size_t\)\(B > 0 \? B : 0\) \* 8 \+ 64;", pp)
    assert re.search(r"ltrx_ndcg_workspace_bytes\(int B, int L\) \{ \(void\)B; \(void\)L; return 0; \}", nd)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# order and ranks (exact)
# ---------------------------------------------------------------------------------------------------------------------------------
def _rank(key, counted, reverse_tie=False):
    """stable descending counting rank of every counted item among the counted ones (ties: the lower index first); -1 elsewhere"""
    idx = np.flatnonzero(counted)
    if reverse_tie:
        idx = idx[::-1]
    rank = np.full(len(key), -1, np.int64)
    rank[idx[np.argsort(-f64(key)[idx], kind="stable")]] = np.arange(len(idx))
    return rank


def _order(rs, valid):
    """order_out of one slate: the valid items by predicted rank, then the padded items in index order"""
    v = np.flatnonzero(valid)
    out = np.empty(len(valid), np.int64)
    out[rs[v]] = v
    out[len(v):] = np.flatnonzero(~valid)
    return out


def _slate_gains(bt, gains):
    if gains is None:
        return [None] * bt.B
    return [np.asarray(gains, F).reshape(bt.s.shape)[b] for b in range(bt.B)]


def visited(bt):
    """[B] bool: the slates a workgroup works on (all of them unless slate_order repeats entries)"""
    out = np.zeros(bt.B, bool)
    out[np.arange(bt.B) if bt.order is None else np.clip(bt.order, 0, bt.B - 1)] = True
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# NDCG
# ---------------------------------------------------------------------------------------------------------------------------------
def _sequences(y, valid, gains, rs, ry):
    """(pred terms, their errors, ideal terms, their errors) by sorted position, in fp64"""
    n = len(y)
    if gains is None:
        g, dg = _gain(np.where(valid, y, F(0)))
    else:
        g, dg = f64(gains), np.zeros(n)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = comp(np.where(g != 0, dg / np.where(g != 0, np.abs(g), 1.0), 0.0), P_LIBM * U, U)
    nv = int(valid.sum())
    pos_p, pos_i = np.where(valid, rs, 0), np.where(valid, ry, 0)
    tail = nv + np.cumsum(~valid) - 1                            # a padded item's position in both rankings
    pos_p, pos_i = np.where(valid, pos_p, tail), np.where(valid, pos_i, tail)
    out = []
    for pos in (pos_p, pos_i):
        t, e = np.zeros(n), np.zeros(n)
        use = valid if gains is None else np.ones(n, bool)
        t[pos[use]] = g[use] / np.log2(pos[use] + 2.0)
        e[pos[use]] = np.abs(t[pos[use]]) * rel[use]
        out += [t, e]
    return out


def ndcg_ref(bt, ats, filler=FILLER, gains=None, entry="ltrx_ndcg_at"):
    T = threads(entry, bt.L)
    ats = np.asarray(ats, np.int64)
    nd, dc, bnd, bdc, orders, fill = [], [], [], [], [], []
    for (s, y, valid), gn in zip(bt.slates(), _slate_gains(bt, gains)):
        n = len(s)
        if n == 0:
            nd.append(np.full(len(ats), float(filler))), dc.append(np.zeros(len(ats))), fill.append(np.ones(len(ats), bool))
            bnd.append(np.zeros(len(ats))), bdc.append(np.zeros(len(ats))), orders.append(np.zeros(0, np.int64))
            continue
        rs, ry = _rank(s, valid), _rank(y, valid)
        orders.append(_order(rs, valid))
        tp, ep, ti, ei = _sequences(y, valid, gn, rs, ry)
        gk = gam(k_scan(n, T))
        at = np.minimum(ats, n) - 1
        d, i_ = np.cumsum(tp)[at], np.cumsum(ti)[at]
        bd = (np.cumsum(ep) + gk * (np.cumsum(np.abs(tp)) + np.cumsum(ep)))[at]
        bi = (np.cumsum(ei) + gk * (np.cumsum(np.abs(ti)) + np.cumsum(ei)))[at]
        zero = np.cumsum(np.abs(ti))[at] == 0
        assert (zero | (np.abs(i_) > 1024 * bi)).all(), "idcg is not clear of 0"
        with np.errstate(invalid="ignore", divide="ignore"):
            q = np.where(zero, float(filler), d / np.where(zero, 1.0, i_))
            bq = np.where(zero, 0.0, (bd + np.abs(q) * bi) / np.where(zero, 1.0, np.abs(i_) - bi))
        nd.append(q), dc.append(d), bnd.append(np.where(zero, 0.0, bq + U * (np.abs(q) + bq))), bdc.append(bd), fill.append(zero)
    return dict(ndcg=np.stack(nd), dcg=np.stack(dc), bar_ndcg=np.stack(bnd), bar_dcg=np.stack(bdc), order=bt.gather(orders, np.int64),
                filler=np.stack(fill), visited=visited(bt))


def ndcg_bar(ref):
    return dict(ndcg=ref["bar_ndcg"], dcg=ref["bar_dcg"])


NDCG_WRONG = ("discount_log2_pos_plus_1", "at_not_clamped", "filler_on_dcg_zero", "tie_reversed", "ideal_order_by_pred_ties",
              "padded_gain_position_off_by_one", "padded_counted_in_rank", "scan_base_by_subtraction")


def ndcg_f32(bt, ats, filler=FILLER, gains=None, entry="ltrx_ndcg_at", wrong=None):
    T = threads(entry, bt.L)
    first = ONE if wrong == "discount_log2_pos_plus_1" else F(2)
    nd, dc, orders = [], [], []
    for (s, y, valid), gn in zip(bt.slates(), _slate_gains(bt, gains)):
        n = len(s)
        if n == 0:
            nd.append(np.full(len(ats), filler, F)), dc.append(np.zeros(len(ats), F)), orders.append(np.zeros(0, np.int64))
            continue
        counted = np.ones(n, bool) if wrong == "padded_counted_in_rank" else valid
        rs = _rank(s, counted, wrong == "tie_reversed")
        ry = _rank(y, counted)
        if wrong == "ideal_order_by_pred_ties":                       # equal labels in predicted order instead of index order
            by = np.flatnonzero(counted)[np.argsort(rs[counted], kind="stable")]
            ry = np.full(n, -1, np.int64)
            ry[by[np.argsort(-f64(y)[by], kind="stable")]] = np.arange(len(by))
        v = np.flatnonzero(valid)
        nv = len(v)
        order = np.full(n, -1, np.int64)
        order[nv:] = np.flatnonzero(~valid)
        dg, ig = np.zeros(n + 1, F), np.zeros(n + 1, F)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            if gn is not None:
                p = nv + np.arange(n - nv) + (1 if wrong == "padded_gain_position_off_by_one" else 0)
                dg[p] = ig[p] = gn[~valid] / np.log2((p.astype(F) + F(2)).astype(F)).astype(F)
                gain = gn[v]
            else:
                gain = (np.exp2(y[v]).astype(F) - ONE).astype(F)
            dg[rs[v]] = gain / np.log2((rs[v].astype(F) + first).astype(F)).astype(F)     # (a colliding rank of a defect: one writer wins)
            ig[ry[v]] = gain / np.log2((ry[v].astype(F) + first).astype(F)).astype(F)
            order[rs[v]] = v
            ext = max(int(np.max(ats)), n)
            ds, is_ = np.zeros(ext, F), np.zeros(ext, F)
            ds[:n] = _scan32(dg[:n], T, by_subtraction=wrong == "scan_base_by_subtraction")
            is_[:n] = _scan32(ig[:n], T, by_subtraction=wrong == "scan_base_by_subtraction")
            at = (np.asarray(ats) if wrong == "at_not_clamped" else np.minimum(ats, n)) - 1
            d, i_ = ds[at], is_[at]
            zero = (d == 0) if wrong == "filler_on_dcg_zero" else (i_ == 0)
            nd.append(np.where(zero, filler, d / i_).astype(F)), dc.append(d)
        orders.append(order)
    out = dict(ndcg=np.stack(nd), dcg=np.stack(dc), order=bt.gather(orders, np.int64))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# MRR
# ---------------------------------------------------------------------------------------------------------------------------------
MRR_WRONG = ("last_maximum", "tie_reversed", "idx_le_at", "zero_rule_per_slate", "padded_ranked", "unvisited_not_cleared")


def _mrr_slates(bt, wrong=None):
    """(best_val [B] fp32, best_idx [B]) -- exact in any precision"""
    bv, bi = np.zeros(bt.B, F), np.zeros(bt.B, np.int32)
    for b, (s, y, valid) in enumerate(bt.slates()):
        n = len(s)
        if n == 0:
            continue
        with np.errstate(invalid="ignore"):
            ss = s.copy() if wrong == "padded_ranked" else np.where(valid, s, F(-np.inf)).astype(F)
        ys = np.where(valid, y, F(0)).astype(F)
        r = _rank(ss, np.ones(n, bool), wrong == "tie_reversed")[ys == ys.max()]
        bv[b], bi[b] = ys.max(), (r.max() if wrong == "last_maximum" else r.min())
    if wrong != "unvisited_not_cleared":
        bv[~visited(bt)], bi[~visited(bt)] = 0, 0
    else:                                                            # what a NaN-filled workspace holds
        bv[~visited(bt)], bi[~visited(bt)] = np.nan, -1
    return bv, bi


def _mrr_out(bv, bi, ats, dtype, wrong=None):
    ats = np.asarray(ats, np.int64)
    tot_zero = (bv == 0) if wrong == "zero_rule_per_slate" else np.full(len(bv), float(f64(bv).sum()) == 0.0)
    r = np.where(tot_zero, dtype(0), dtype(1) / (bi.astype(dtype) + dtype(1))).astype(dtype)
    inside = (bi[:, None] <= ats[None, :]) if wrong == "idx_le_at" else (bi[:, None] < ats[None, :])
    return np.where(inside, r[:, None], dtype(0)).astype(dtype)


def mrr_ref(bt, ats):
    bv, bi = _mrr_slates(bt)
    out = _mrr_out(bv, bi, ats, np.float64)
    return dict(mrr=out, bar_mrr=U * np.abs(out), best_val=bv, best_idx=bi)


def mrr_bar(ref):
    return dict(mrr=ref["bar_mrr"])


def mrr_f32(bt, ats, wrong=None):
    bv, bi = _mrr_slates(bt, wrong)
    return dict(mrr=_mrr_out(bv, bi, ats, F, wrong), best_val=bv, best_idx=bi)


# ---------------------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name entry L ats draw order")       # draw: the input recipe; order: None / "perm" / "longest" / "repeat"

PADDED_L = (1, 2, 3, 255, 256, 257, 512, 513, 3072, 3073, 8192)
MRR_EXTRA_L = (6144, 6145)
MANY_ATS_L = (3, 257, 513)


def ats_of(L, n_ats):
    """cut-offs holding 1, the slate length and values above it"""
    if n_ats == 1:
        return (5,)
    if n_ats == 3:
        return (1, L, L + 5)
    return (1, 2, 3, 4, 5, 7, 10, 16, 31, 32, 33, 64, 100, L, L + 1, 2 * L + 3)


def _cases():
    out = []

    def add(entry, L, n_ats, draw="grid", order=None, ats=None):
        ats = ats_of(L, n_ats) if ats is None else ats
        out.append(Case("%s L %d ats %d %s%s" % (entry, L, len(ats), draw, "" if order is None else " order " + order), entry, L, ats, draw, order))

    for L in PADDED_L:
        for n_ats in (1, 3, 16) if L in MANY_ATS_L else (3,):
            add("ltrx_ndcg_at", L, n_ats)
            add("ltrx_mrr_at", L, n_ats)
    for L in MRR_EXTRA_L:
        add("ltrx_mrr_at", L, 3)
    add("ltrx_mrr_at", 3, 3, "zero batch")                       # every maximum label 0: the whole result is zeroed
    for L in (3, 257):
        add("ltrx_ndcg_at_gains", L, 3, "gain y+1")              # gain_function(0) = 1: the padded tail carries gains
    add("ltrx_ndcg_at_gains", 257, 16, "signed item gains")
    add("ltrx_ndcg_at_gains", 3072, 3, "wide item gains", ats=(4, 3072, 4000))
    for L in (256, 257):
        for order in (None, "perm", "longest"):
            add("ltrx_ndcg_at_cu", L, 3, "ragged", order, ats=(1, 5, 10, 300))
            add("ltrx_mrr_at_cu", L, 3, "ragged", order, ats=(1, 5, 10, 300))
    add("ltrx_ndcg_at_cu", 257, 16, "ragged", "repeat")          # unvisited slates keep what the output held
    add("ltrx_mrr_at_cu", 257, 3, "ragged", "repeat", ats=(1, 5, 10, 300))   # unvisited slates count as empty: (0, 0), cleared by the call
    add("ltrx_ndcg_at_cu", 257, 1, "ragged", "perm")
    add("ltrx_mrr_at_cu", 257, 16, "ragged", "perm")
    add("ltrx_ndcg_at_cu", 3073, 3, "ragged long", "longest")
    add("ltrx_mrr_at_cu", 3073, 3, "ragged long", "perm")
    return out


CASES = _cases()
Inputs = namedtuple("Inputs", "bt gains")


def valid_counts(L):
    """leading valid items per slate: full; 1 valid item; fully padded; half (tie-heavy scores); full with labels all 0 -- two slates (full
    with tie-heavy scores, a little more than half) from 3072 on"""
    if L >= 3072:
        return (L, L // 2 + 1)
    return (L, 1, 0, max(1, L // 2), L)


@functools.lru_cache(maxsize=None)
def _inputs(draw, L):
    rng = np.random.default_rng([sum(map(ord, draw)), L])
    if draw.startswith("ragged"):
        lengths = (5, 0, L, 1, 100) if draw == "ragged long" else tuple(n for n in RAGGED_LENGTHS if n <= L)
        ss, ys = [], []
        for b, n in enumerate(lengths):
            s, y = rng.standard_normal(n), rng.integers(0, 5, n).astype(np.float64)
            if b in (7, 10) or n > 257:
                s = np.round(s * 10) / 10                        # tie-heavy
            elif n >= 2:
                s[-1] = s[0]
            if b == 5:
                y[:] = 0                                         # idcg == 0
            ss.append(s), ys.append(y)
        cu = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
        bt = Batch(np.concatenate(ss).astype(F), np.concatenate(ys).astype(F), cu, None, L)
        return Inputs(bt, None)
    counts = valid_counts(L)
    B = len(counts)
    s = rng.standard_normal((B, L))                              # padded slots keep a score of their own: a kernel must not rank them
    y = rng.integers(0, 5, (B, L)).astype(np.float64)
    for b, nv in enumerate(counts):
        if b == (3 if B == 5 else 0):
            s[b] = np.round(s[b] * 10) / 10
        elif nv >= 2:
            s[b, nv - 1] = s[b, 0]
        if b == 4 or draw == "zero batch":
            y[b] = 0
        y[b, nv:] = float(PAD)
    s, y = s.astype(F), y.astype(F)
    gains = None
    if draw == "gain y+1":
        gains = (np.where(y == PAD, F(0), y) + ONE).astype(F)
    elif draw == "signed item gains":                            # per item, of both signs; the top labels carry the large ones: idcg far from 0
        gains = (rng.standard_normal((B, L)) + 3.0 * np.where(y == PAD, 0, y)).astype(F)
    elif draw == "wide item gains":                              # the four items ranked first by the scores: 1e-6; every other about 1e3
        gains = (1e3 * rng.uniform(0.5, 1.0, (B, L))).astype(F)
        for b in range(B):
            v = np.flatnonzero(y[b] != PAD)
            top = v[np.argsort(-f64(s[b])[v], kind="stable")[:4]]
            gains[b, top] = F(1e-6) * (1 + np.arange(4)).astype(F)
    return Inputs(Batch(s, y), gains)


def slate_order(c, bt):
    if c.order is None:
        return None
    n = np.diff(bt.cu)
    if c.order == "longest":
        return np.argsort(-n, kind="stable").astype(np.int32)
    perm = np.random.default_rng([bt.B, c.L]).permutation(bt.B).astype(np.int32)
    if c.order == "repeat":
        perm[1], perm[-1] = perm[0], perm[2]                     # two slates twice, two never
    return perm


def inputs(c):
    """the case's (Batch, gains): scores N(0, 1) in fp32 with exact ties (one slate rounded to 0.1, every other repeats its first score
    at its last valid item), integer labels 0..4 (every count far below 2^24), padded tails of different lengths whose slots hold
    scores of their own, one slate of zero labels"""
    base = _inputs(c.draw, c.L)
    bt = base.bt
    assert bt.L == c.L and bt.s.size < 2 ** 24
    if bt.ragged:
        bt = Batch(bt.s, bt.y, bt.cu, slate_order(c, bt), c.L)
    if base.gains is not None and c.draw != "signed item gains":
        assert (base.gains >= 0).all()
    bt.s.setflags(write=False), bt.y.setflags(write=False)
    return Inputs(bt, base.gains)


def is_mrr(c):
    return c.entry in MRR_ENTRIES


@functools.lru_cache(maxsize=None)
def reference(c):
    i = inputs(c)
    return mrr_ref(i.bt, c.ats) if is_mrr(c) else ndcg_ref(i.bt, c.ats, FILLER, i.gains, c.entry)


def transcription(c, wrong=None):
    i = inputs(c)
    return mrr_f32(i.bt, c.ats, wrong) if is_mrr(c) else ndcg_f32(i.bt, c.ats, FILLER, i.gains, c.entry, wrong)


def checks(c, got, ref=None):
    """{output: (got, ref, bar)} of the floating-point outputs, over the slates a workgroup visits"""
    ref = reference(c) if ref is None else ref
    if is_mrr(c):
        return dict(mrr=(got["mrr"], ref["mrr"], ref["bar_mrr"]))
    v = ref["visited"]
    out = dict(ndcg=(np.asarray(got["ndcg"])[v], ref["ndcg"][v], ref["bar_ndcg"][v]))
    if "dcg" in got:
        out["dcg"] = (np.asarray(got["dcg"])[v], ref["dcg"][v], ref["bar_dcg"][v])
    return out


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def exact_ok(c, got, ref=None):
    """the outputs compared bit for bit: order_out over every visited slate, the filler entries, a 0 DCG; for MRR (best_val, best_idx) and
    the whole output against the fp32 transcription"""
    ref = reference(c) if ref is None else ref
    bt = inputs(c).bt
    if is_mrr(c):
        want = mrr_f32(bt, c.ats)
        return bool(np.array_equal(_bits(got["mrr"]), _bits(want["mrr"])) and np.array_equal(_bits(got["best_val"]), _bits(ref["best_val"]))
                    and np.array_equal(np.asarray(got["best_idx"], np.int64), np.asarray(ref["best_idx"], np.int64)))
    v = ref["visited"]
    fill = ref["filler"] & v[:, None]
    ok = np.array_equal(_bits(np.asarray(got["ndcg"])[fill]), _bits(np.full(int(fill.sum()), FILLER)))
    if "order" in got:
        rows = np.repeat(v, bt.L).reshape(bt.s.shape) if not bt.ragged else np.repeat(v, np.diff(bt.cu))
        ok = ok and np.array_equal(np.asarray(got["order"])[rows], ref["order"][rows])
    return bool(ok)


def applies(c, wrong):
    """None if the defect can show on this case, else why it cannot"""
    bt = inputs(c).bt
    ragged = bt.ragged
    if wrong in ("padded_counted_in_rank", "padded_ranked", "padded_gain_position_off_by_one") and ragged:
        return "no padded items"
    if wrong == "padded_gain_position_off_by_one" and c.entry != "ltrx_ndcg_at_gains":
        return "padded items carry a gain only in the gains form"
    if wrong == "ideal_order_by_pred_ties" and c.draw not in ("signed item gains", "wide item gains"):
        return "a gain that is a function of the label: the ideal DCG sums the same multiset"
    if wrong == "scan_base_by_subtraction" and c.draw != "wide item gains":
        return "positive terms of one size: the difference is rounded at the size of the entry itself"
    if wrong == "at_not_clamped" and max(c.ats) <= (min(len(s) for s, _, _ in bt.slates()) if ragged else c.L):
        return "no cut-off above a slate"
    if wrong in ("tie_reversed", "last_maximum", "filler_on_dcg_zero", "padded_counted_in_rank", "padded_ranked") and c.L < 3:
        return "too short for a tie, a second maximum or a padded item next to two valid ones"
    if wrong == "unvisited_not_cleared" and c.order != "repeat":
        return "every slate is visited"
    if wrong == "zero_rule_per_slate" and c.draw == "zero batch":
        return "every slate is zero"
    return None


WRONG = {e: NDCG_WRONG for e in NDCG_ENTRIES}
WRONG.update({e: MRR_WRONG for e in MRR_ENTRIES})
