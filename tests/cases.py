"""Shared enumeration of the golden loss cases (tests/golden/losses_golden.npz, made by make_golden.py)."""
LAMBDA_SCHEMES = [None, "ndcgLoss1_scheme", "ndcgLoss2_scheme", "lambdaRank_scheme", "ndcgLoss2PP_scheme",
                  "rankNet_scheme", "rankNetWeightedByGTDiff_scheme", "rankNetWeightedByGTDiffPowed_scheme"]


def close(a, b, rtol=1e-5, atol=1e-5):
    """|a-b| <= atol + rtol*|b| -- the 1e-5 fp32 bar of BASELINE.json's north_star, relative for large values."""
    import numpy as np
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    both_nan = np.isnan(a) & np.isnan(b)      # e.g. lambdaLoss(reduction="mean") over an empty pair selection
    return bool(np.all(both_nan | (np.abs(a - b) <= atol + rtol * np.abs(b))))


def grad_close(g, gref, rtol=2e-4):
    """gradient check: max abs error relative to the largest reference gradient entry of the tensor."""
    import numpy as np
    g = np.asarray(g, dtype=np.float64)
    gref = np.asarray(gref, dtype=np.float64)
    scale = max(float(np.abs(gref).max()), 1e-6)
    return float(np.abs(g - gref).max()) <= rtol * scale + 1e-7


def iter_loss_cases(gold):
    """yields (name, kind, kwargs, s, y, ref_loss, ref_grad)"""
    n = int(gold["n_cases"])
    for ci in range(n):
        pre = "c%d." % ci
        s, y = gold[pre + "s"], gold[pre + "y"]
        yield (pre + "listnet", "listnet", {}, s, y, gold[pre + "listnet.loss"], gold[pre + "listnet.grad"])
        for a in (1.0, 2.5):
            k = pre + "approxndcg.a%g" % a
            yield (k, "approxndcg", dict(alpha=a), s, y, gold[k + ".loss"], gold[k + ".grad"])
        yield (pre + "listmle", "listmle", dict(perm=gold[pre + "listmle.perm"]), s, y,
               gold[pre + "listmle.loss"], gold[pre + "listmle.grad"])
        for si, sch in enumerate(LAMBDA_SCHEMES):
            for kk in (None, 5):
                for red, lg in (("sum", "binary"), ("mean", "natural")):
                    k = pre + "lambda.s%d.k%s.%s.%s" % (si, kk, red, lg)
                    yield (k, "lambdaloss", dict(weighing_scheme=sch, k=kk, reduction=red, reduction_log=lg, sigma=1.3, mu=7.0),
                           s, y, gold[k + ".loss"], gold[k + ".grad"])
        for tr in (False, True):
            for tau in (1.0, 0.1):
                for kk in (None, 5):
                    for pw in (True, False):
                        k = pre + "neural.t%d.tau%g.k%s.p%d" % (int(tr), tau, kk, int(pw))
                        yield (k, "neuralndcg", dict(transposed=tr, temperature=tau, k=kk, powered_relevancies=pw),
                               s, y, gold[k + ".loss"], gold[k + ".grad"])


# ---- SURVEY.md section 8f row 4 fixtures (tests/golden/extra_golden.npz, made by make_golden_extra.py) ----
STOCH = [dict(tr=False, tau=1.0, k=None, pw=True, log=True, beta=0.1), dict(tr=False, tau=0.5, k=5, pw=False, log=False, beta=0.3),
         dict(tr=True, tau=1.0, k=None, pw=True, log=True, beta=0.1), dict(tr=True, tau=2.0, k=7, pw=False, log=True, beta=1.0)]
N_ORD = 4


def iter_extra_cases(gold):
    """yields (name, kind, kwargs, y_pred, y_true, ref_loss, ref_grad) for the pointwise / pairwise losses"""
    for ci in range(int(gold["n_cases"])):
        pre = "c%d." % ci
        s, y = gold[pre + "s"], gold[pre + "y"]
        for m, kw in enumerate((dict(), dict(weight_by_diff=True), dict(weight_by_diff_powed=True))):
            yield (pre + "ranknet.m%d" % m, "ranknet", kw, s, y, gold[pre + "ranknet.m%d.loss" % m], gold[pre + "ranknet.m%d.grad" % m])
        yield (pre + "bce.nopad", "bce", {}, gold[pre + "pe"], gold[pre + "ybnp"], gold[pre + "bce.nopad.loss"], gold[pre + "bce.nopad.grad"])
        yield (pre + "bce.pad", "bce", {}, gold[pre + "p"], gold[pre + "yb"], gold[pre + "bce.pad.loss"], gold[pre + "bce.pad.grad"])
        yield (pre + "ordinal.nopad", "ordinal", dict(n=N_ORD), gold[pre + "p3e"], gold[pre + "ynp"],
               gold[pre + "ordinal.nopad.loss"], gold[pre + "ordinal.nopad.grad"])
        yield (pre + "ordinal.pad", "ordinal", dict(n=N_ORD), gold[pre + "p3"], y, gold[pre + "ordinal.pad.loss"], gold[pre + "ordinal.pad.grad"])
        yield (pre + "rmse", "pointwise_rmse", dict(no_of_levels=4), gold[pre + "p"], y, gold[pre + "rmse.loss"], gold[pre + "rmse.grad"])
        yield (pre + "blistnet", "binary_listnet", {}, s, gold[pre + "yb"], gold[pre + "blistnet.loss"], gold[pre + "blistnet.grad"])


def iter_stochastic_cases(gold):
    """yields (name, cfg, s, y, gumbel[S,B,L], ref_loss, ref_grad, strict_mask): ``strict_mask`` excludes the batch-minimum
    score(s) when log_scores is on -- there d log(s - min + 1e-10)/ds = 1e10 amplifies fp32 round-off in the reference too."""
    for ci in range(int(gold["n_cases"])):
        pre = "c%d." % ci
        s, y = gold[pre + "s"], gold[pre + "y"]
        for si, c in enumerate(STOCH):
            strict = (s != s.min()) if c["log"] else (s == s)
            yield (pre + "stoch%d" % si, c, s, y, gold[pre + "gumbel"][..., 0], gold[pre + "stoch%d.loss" % si],
                   gold[pre + "stoch%d.grad" % si], strict)


def row4_kats():
    """the known-answer tests of /root/reference/tests/losses/test_{ranknet,mrr,loss_ordinal,loss_pointwise,binary_listnet}.py
    restated as (kind, kwargs, y_pred, y_true, expected): expected values come from the same independent closed forms the
    reference tests use (BCE-with-logits of the score differences, cross-entropy by hand, ...)."""
    import math
    import numpy as np

    def bcel(ds, ws=None):                                     # BCEWithLogitsLoss(weight)(ds, ones), mean
        ws = ws or [1.0] * len(ds)
        return float(np.mean([w * math.log1p(math.exp(-d)) for d, w in zip(ds, ws)]))

    def xe(t, p):
        return -t * math.log(p) - (1 - t) * math.log(1 - p)

    def sm(v):
        e = np.exp(np.asarray(v, np.float64) - np.max(v))
        return e / e.sum()

    P = -1.0
    k = []
    # test_ranknet.py:29-115
    k += [("ranknet", {}, [0.5, 0.2], [1.0, 0.0], bcel([0.3])), ("ranknet", {}, [0.2, 0.5], [1.0, 0.0], bcel([-0.3])),
          ("ranknet", {}, [0.5, 0.2, 0.1], [1.0, 0.0, 0.0], bcel([0.3, 0.4])), ("ranknet", {}, [0.2, 0.5], [0.0, 1.0], bcel([0.3])),
          ("ranknet", {}, [0.2, 0.5], [0.0, 2.0], bcel([0.3])), ("ranknet", {}, [0.5, 0.2, 0.66], [1.0, 0.0, P], bcel([0.3])),
          ("ranknet", dict(weight_by_diff=True), [0.5, 0.2, 0.1], [2.0, 1.0, 0.0], bcel([0.3, 0.4, 0.1], [1.0, 2.0, 1.0])),
          ("ranknet", dict(weight_by_diff_powed=True), [0.5, 0.2, 0.1], [2.0, 1.0, 0.0], bcel([0.3, 0.4, 0.1], [3.0, 4.0, 1.0]))]
    # test_loss_ordinal.py:28-58 (n = 2)
    k += [("ordinal", dict(n=2), [[0.8, 0.6]], [1.0], xe(1, 0.8) + xe(0, 0.6)),
          ("ordinal", dict(n=2), [[0.8, 0.7], [0.4, 0.3], [0.2, 0.1]], [2.0, 1.0, 0.0],
           float(np.mean([xe(1, 0.8) + xe(1, 0.7), xe(1, 0.4) + xe(0, 0.3), xe(0, 0.2) + xe(0, 0.1)]))),
          ("ordinal", dict(n=2), [[0.8, 0.6], [0.2, 0.1]], [1.0, P], xe(1, 0.8) + xe(0, 0.6))]
    # test_loss_pointwise.py:16-47
    k += [("pointwise_rmse", dict(no_of_levels=1), [0.5, 0.2], [1.0, 0.0], math.sqrt(np.mean([0.25, 0.04]))),
          ("pointwise_rmse", dict(no_of_levels=1), [0.5, 0.2, 0.5], [1.0, 0.0, P], math.sqrt(np.mean([0.25, 0.04]))),
          ("pointwise_rmse", dict(no_of_levels=3), [0.5, 0.2, 0.7, 0.8], [1.0, 0.0, 2.0, 3.0],
           math.sqrt(np.mean([0.25, 0.36, 0.01, 0.36])))]
    # test_binary_listnet.py:16-47
    k += [("binary_listnet", dict(eps=0.0), [0.5, 0.2], [1.0, 0.0], float(-np.log(sm([0.5, 0.2])[0]))),
          ("binary_listnet", {}, [0.5, -1e30], [1.0, 0.0], float(-np.log(sm([0.5, -1e30])[0] + 1e-10))),
          ("binary_listnet", {}, [0.5, 0.2, 0.5], [1.0, 0.0, P], float(-np.log(sm([0.5, 0.2])[0] + 1e-10)))]
    return k


def mrr_kats():
    """test_mrr.py:19-105 as (y_pred rows, y_true rows, ats, expected matrix)"""
    P = -1.0
    return [([[0.5, 0.2]], [[1.0, 0.0]], [10], [[1.0]]), ([[0.5, 0.2]], [[1.0, 0.0]], None, [[1.0]]),
            ([[0.5, 0.2]], [[0.0, 1.0]], [10], [[0.5]]),
            ([[0.2, 0.5], [0.5, 0.2]], [[0.0, 1.0], [0.0, 1.0]], [10], [[1.0], [0.5]]),
            ([[0.5, 0.2]], [[0.0, 1.0]], [1, 2], [[0.0, 0.5]]),
            ([[0.2, 0.5], [0.5, 0.2]], [[0.0, 1.0], [0.0, 1.0]], [1, 2], [[1.0, 1.0], [0.0, 0.5]]),
            ([[0.5, 0.2]], [[0.0, 0.0]], [10], [[0.0]]),
            ([[0.5, 0.2, 1.0]], [[1.0, 0.0, P]], [10], [[1.0]]), ([[0.5, 0.2, 1.0]], [[0.0, 1.0, P]], [10], [[0.5]])]


# ---- score-scale fixtures (tests/golden/scale_golden.npz, made by make_golden_scale.py) ----
# A model in training does not emit N(0, 1) scores: the slates above, multiplied by these factors, reach the clamp / eps branches
# of every listwise loss (sigmoid(alpha * diff) saturating, log(P + eps), q^w >= eps, near one-hot NeuralSort).
SCALES = (1, 8, 30, 100, 1000)
# (name, B, L, seed, tie_scores, full case matrix?)
SCALE_SETS = (("main", 4, 240, 13, False, True), ("ties", 3, 33, 14, True, True), ("outlier", 3, 50, 15, False, True),
              ("tiny", 6, 3, 16, False, True), ("long", 2, 1024, 17, False, False))


def scale_inputs(B, L, seed, ties, name):
    """the unscaled slate of a set: make_inputs, plus for "outlier" one item per slate 50 above the rest of it"""
    from tests.golden.make_inputs import make_inputs
    s, y = make_inputs(B, L, seed, ties)
    if name == "outlier":
        for b in range(B):
            nv = int((y[b] != -1).sum())
            s[b, (7 * b + 3) % nv] += 50.0
    return s, y


def scale_loss_cases(full):
    """[(case name, kind, kwargs)] -- the perm of listMLE and the binary labels of binary listNet come from the fixture"""
    cases = [("listnet", "listnet", {}), ("listmle", "listmle", {}), ("approxndcg.a1", "approxndcg", dict(alpha=1.0))]
    if full:
        cases.append(("approxndcg.a2.5", "approxndcg", dict(alpha=2.5)))
    lam = [(si, None, "sum", "binary") for si in range(len(LAMBDA_SCHEMES))] + [(si, 5, "mean", "natural") for si in range(len(LAMBDA_SCHEMES))]
    if not full:
        lam = [(3, None, "sum", "binary"), (4, 5, "mean", "natural")]
    for si, kk, red, lg in lam:
        cases.append(("lambda.s%d.k%s.%s.%s" % (si, kk, red, lg), "lambdaloss",
                      dict(weighing_scheme=LAMBDA_SCHEMES[si], k=kk, reduction=red, reduction_log=lg, sigma=1.3, mu=7.0)))
    neural = [(tr, tau, kk, True) for tr in (False, True) for tau in (1.0, 0.1) for kk in (None, 5)] + \
             [(False, 1.0, None, False), (True, 1.0, None, False)]
    if not full:
        neural = [(False, 1.0, None, True), (True, 0.1, 5, True)]
    for tr, tau, kk, pw in neural:
        cases.append(("neural.t%d.tau%g.k%s.p%d" % (int(tr), tau, kk, int(pw)), "neuralndcg",
                      dict(transposed=tr, temperature=tau, k=kk, powered_relevancies=pw)))
    if full:
        for m, kw in enumerate((dict(), dict(weight_by_diff=True), dict(weight_by_diff_powed=True))):
            cases.append(("ranknet.m%d" % m, "ranknet", kw))
        cases.append(("blistnet", "binary_listnet", {}))
    return cases


SCALE_NDCG_ATS = (1, 5, 10)         # + L
SCALE_MRR_ATS = (1, 10)


def iter_scale_cases(gold):
    """yields (set name, scale, case name, kind, kwargs, s, y, ref_loss, ref_grad): s already multiplied by the scale, y the binary
    labels for binary listNet; kwargs of listMLE carry the recorded perm"""
    for name, B, L, seed, ties, full in SCALE_SETS:
        for sc in SCALES:
            pre = "%s.x%d." % (name, sc)
            s, y = gold[pre + "s"], gold[name + ".y"]
            for cname, kind, kw in scale_loss_cases(full):
                kw = dict(kw)
                yy = y
                if kind == "listmle":
                    kw["perm"] = gold[name + ".perm"]
                elif kind == "binary_listnet":
                    yy = gold[name + ".yb"]
                yield name, sc, cname, kind, kw, s, yy, gold[pre + cname + ".loss"], gold[pre + cname + ".grad"]


def neural_scale_check(loss, grad, ref_loss, ref_grad, loss64, grad64):
    """the conditioning-aware NeuralNDCG bar at score scale: at |s| >> 1 the NeuralSort logits (L+1-2i) s_j - sum_k |s_j - s_k|
    cancel and the reference's own fp32 gradient moves away from the fp64 oracle by up to ~10x its largest entry, so the anchor is
    the fp64 oracle and the bar grows with the reference's own fp32 error:
        max|g - g64| <= max(5e-4 max|g64|, 4 max|g_ref32 - g64|) + 1e-12,   |l - l64| <= max(1e-5 (1 + |l64|), 4 |l_ref32 - l64|).
    returns (ok, row of the measured errors)"""
    import numpy as np
    g, g64 = np.asarray(grad, np.float64), np.asarray(grad64, np.float64)
    e_ref = float(np.abs(np.asarray(ref_grad, np.float64) - g64).max())
    err = float(np.abs(g - g64).max())
    gbar = max(5e-4 * float(np.abs(g64).max()), 4 * e_ref) + 1e-12
    l_ref = abs(float(ref_loss) - float(loss64))
    lerr = abs(float(loss) - float(loss64))
    lbar = max(1e-5 * (1 + abs(float(loss64))), 4 * l_ref)
    ok = bool(np.isfinite(g).all() and np.isfinite(loss) and err <= gbar and lerr <= lbar)
    return ok, dict(gerr=err, gbar=gbar, e_ref=e_ref, g64max=float(np.abs(g64).max()), lerr=lerr, lbar=lbar, l_ref=l_ref)
