"""The ragged batch of tests/test_ragged_cpu.py and tests/test_gpu_ragged.py and its fp64 expectations.

One batch: slates of 0, 1, 2, 3, 5, 31, 32, 33, 64, 100, 255, 256 and 257 items (empty; shorter than a wave; either side of 32 / 64 /
256, the widths of a wave and of the kernels' item stride), integer labels 0..4 (ties in the labels everywhere), one slate with only
zero labels, and scores with exact ties: two slates are quantised to quarters, every other slate repeats its first score at its
last item.  The scores are fp32 values (times the score scale, in fp32); the oracle evaluates exactly those values in fp64.

Expected values come from oracle/ltr_oracle.py on the PADDED grid [B, L]: every slate's items first, label -1 and score 0 after
them.  The only place where the oracle has no value for an empty slate is listNet (softmax over nothing: NaN); its contribution is
0 by the library's definition (ltrx_listnet.hip, "a fully padded slate"), applied in ``listnet_expected``."""
import numpy as np

from oracle import ltr_oracle as O
from tests.cases import LAMBDA_SCHEMES

LENGTHS = (0, 1, 2, 3, 5, 31, 32, 33, 64, 100, 255, 256, 257)
ZERO_LABEL_SLATE = 5            # the slate of 31 items
QUANTISED = (7, 10)             # slates of 33 and 255 items: scores in quarters -> many exact ties
ATS = [1, 5, 10, 300]
PAD_WIDTHS = (257, 921)         # the batch's own maximum, and the width of the r07 validation set
LAMBDA_CASES = [(sch, k, red, lg) for sch in LAMBDA_SCHEMES for k in (None, 5) for red, lg in (("sum", "binary"), ("mean", "natural"))]
LAMBDA_KW = dict(sigma=1.3, mu=7.0)


def make_batch(scale=1, seed=20, lengths=LENGTHS):
    """(scores[n] fp32, labels[n] fp32, cu[B+1] int32)"""
    rng = np.random.RandomState(seed)
    ss, ys = [], []
    for b, n in enumerate(lengths):
        s = rng.randn(n).astype(np.float32)
        y = rng.randint(0, 5, size=n).astype(np.float32)
        if b in QUANTISED:
            s = (np.round(s * 4) / 4).astype(np.float32)
        elif n >= 2:
            s[-1] = s[0]
        if b == ZERO_LABEL_SLATE:
            y[:] = 0
        ss.append(s)
        ys.append(y)
    cu = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    s = (np.concatenate(ss) * np.float32(scale)).astype(np.float32)
    return s, np.concatenate(ys).astype(np.float32), cu


def to_grid(v, cu, L, fill):
    """packed [n] -> padded [B, L], every slate's items first"""
    B = len(cu) - 1
    g = np.full((B, L), fill, dtype=np.float64)
    for b in range(B):
        g[b, :cu[b + 1] - cu[b]] = v[cu[b]:cu[b + 1]]
    return g


def to_packed(g, cu):
    """padded [B, L] -> packed [n]"""
    return np.concatenate([g[b, :cu[b + 1] - cu[b]] for b in range(len(cu) - 1)]) if cu[-1] else g[:0, 0]


def grids(s, y, cu, L):
    return to_grid(s, cu, L, 0.0), to_grid(y, cu, L, -1.0)


def listnet_expected(sg, yg, cu):
    """(loss, packed gradient, per-slate) with an empty slate's contribution defined as 0"""
    with np.errstate(all="ignore"):
        _, grad, per = O.listnet(sg, yg, dtype=np.float64)
    per = np.where(np.diff(cu) == 0, 0.0, per)
    return float(per.sum() / len(per)), to_packed(np.nan_to_num(grad), cu), per


def approxndcg_expected(sg, yg, cu, alpha=1.0):
    with np.errstate(all="ignore"):
        loss, grad, per = O.approxndcg(sg, yg, alpha=alpha, dtype=np.float64)
    return float(loss), to_packed(grad, cu), per


def lambdaloss_expected(sg, yg, cu, sch, k, red, lg):
    """(loss, packed gradient, selected pairs, packed in-slate order)"""
    with np.errstate(all="ignore"):
        loss, grad, n_sel, ip = O.lambdaloss(sg, yg, weighing_scheme=sch, k=k, reduction=red, reduction_log=lg, dtype=np.float64, **LAMBDA_KW)
    return float(loss), to_packed(grad, cu), n_sel, to_packed(ip, cu)


def metrics_expected(sg, yg, cu, ats=ATS, filler=1.0):
    """ndcg, dcg [B, len(ats)], packed in-slate order, mrr [B, len(ats)]"""
    with np.errstate(all="ignore"):
        nd, order = O.ndcg(sg, yg, ats=ats, filler_value=filler, dtype=np.float64)
        dc, _ = O.dcg(sg, yg, ats=ats, dtype=np.float64)
        mr = O.mrr(sg, yg, ats=ats, dtype=np.float64)
    return nd, dc, to_packed(order, cu), mr


def expected(scale, L=PAD_WIDTHS[0]):
    """everything the GPU tests compare against, for one score scale, from the grid of width L"""
    s, y, cu = make_batch(scale)
    sg, yg = grids(s, y, cu, L)
    out = {"s": s, "y": y, "cu": cu, "listnet": listnet_expected(sg, yg, cu), "approxndcg": approxndcg_expected(sg, yg, cu),
           "metrics": metrics_expected(sg, yg, cu), "metrics_f0": metrics_expected(sg, yg, cu, filler=0.25)}
    for c in LAMBDA_CASES:
        out[("lambda",) + c] = lambdaloss_expected(sg, yg, cu, *c)
    return out
