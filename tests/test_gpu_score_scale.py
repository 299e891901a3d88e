"""The loss and metric kernels at the score scales of a model in training (-m gpu).  Every other parity test feeds N(0, 1) scores; a
model in training reaches |s| ~ 30 within a few steps, where the clamp / eps branches decide the result: approxNDCG's sigmoid of
alpha * diff in the hundreds (exp overflow, rcp(inf) = 0, clamp(min=eps)), lambdaLoss's max(sigmoid, eps) / max(q^w, eps) and the
``live`` flag of its gradient, log(P + eps) of listNet and binary listNet, log(C + eps) of listMLE, a near one-hot NeuralSort
matrix meeting Sinkhorn's clamps.  Fixture: tests/golden/scale_golden.npz (make_golden_scale.py) -- the golden slates with their
scores multiplied by 1, 8, 30, 100 and 1000; scale 1 is the control.

Bars: the non-NeuralNDCG losses are held to the scale-1 bars at every scale (loss 1e-5, gradient 2e-4 of its largest reference
entry, padded entries exactly 0, everything finite).  NeuralNDCG is ill-conditioned at scale in the reference itself, so its anchor
is the fp64 oracle and its bar grows with the reference's own fp32 error (tests/cases.py neural_scale_check)."""
import os

import numpy as np
import pytest
import torch

from oracle import ltr_oracle as O
from tests.cases import SCALES, SCALE_SETS, SCALE_MRR_ATS, SCALE_NDCG_ATS, close, grad_close, iter_scale_cases, neural_scale_check
from tests.test_gpu_parity import _engine_loss, _log, _t

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = {name: (B, L) for name, B, L, seed, ties, full in SCALE_SETS}


@pytest.fixture(scope="module")
def scale_golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "scale_golden.npz"), allow_pickle=False))


def _engine(kind, kw, s, y):
    from allrank_amd import losses as E
    if kind in ("ranknet", "binary_listnet"):
        sp = _t(s, True)
        l = (E.rankNet if kind == "ranknet" else E.binary_listNet)(sp, _t(y), **kw)
        l.backward()
        return float(l.item()), sp.grad.cpu().numpy()
    return _engine_loss(kind, kw, s, y)


@pytest.mark.parametrize("scale", SCALES)
def test_losses_match_reference_at_score_scale(scale, scale_golden):
    rows, bad = [], []
    for st, sc, cname, kind, kw, s, y, rl, rg in iter_scale_cases(scale_golden):
        if sc != scale or kind == "neuralndcg":
            continue
        lo, go = _engine(kind, kw, s, y)
        gerr, gmax = float(np.abs(go - rg).max()), float(np.abs(rg).max())
        ok = (np.isfinite(lo) or np.isnan(rl)) and np.isfinite(go).all() and close(lo, rl) and grad_close(go, rg) and np.all(go[y == -1] == 0)
        rows.append(dict(case="%s.%s" % (st, cname), loss=lo, ref=float(rl), gerr=gerr, gmax=gmax, grel=gerr / max(gmax, 1e-6), ok=bool(ok)))
        if not ok:
            bad.append(rows[-1])
    _log("score_scale_losses_x%d" % scale, rows)
    assert len(rows) == 4 * 24 + 5 and not bad, bad[:8]


@pytest.mark.parametrize("scale", SCALES)
def test_neuralndcg_both_paths_within_the_conditioning_bar_at_score_scale(scale, scale_golden):
    """NeuralNDCG and its transposed form vs the fp64 oracle, computed here; slates of L <= 240 through both the block-resident
    kernels (path 0) and the general L2-streaming kernels (path 1), L = 1024 through the general ones"""
    from allrank_amd import losses as E
    rows, bad = [], []
    for st, sc, cname, kind, kw, s, y, rl, rg in iter_scale_cases(scale_golden):
        if sc != scale or kind != "neuralndcg":
            continue
        l64, g64 = O.neuralndcg(s, y, dtype=np.float64, **kw)[:2]
        for path in ((0, 1) if s.shape[1] <= 240 else (0,)):
            with E.neural_kernel_path(path):
                lo, go = _engine_loss(kind, kw, s, y)
            ok, row = neural_scale_check(lo, go, rl, rg, l64, g64)
            ok = ok and bool(np.all(go[y == -1] == 0))
            row.update(case="%s.%s" % (st, cname), path=path, loss=lo, ok=ok)
            rows.append(row)
            if not ok:
                bad.append(row)
    _log("score_scale_neuralndcg_x%d" % scale, rows)
    assert len(rows) == 4 * 10 * 2 + 2 and not bad, bad[:8]


@pytest.mark.parametrize("scale", [30, 1000])
def test_fused_loss_equals_the_plugin_call_at_score_scale(scale, scale_golden):
    """FusedLoss (the explicit training step's loss launcher) == the autograd plugin call, bit for bit, for every loss name FusedLoss
    accepts.  The ranking losses on trained-scale scores (listMLE with one explicit permutation on both paths, binary listNet on the
    binary labels); bce, ordinal and pointwise_rmse take probabilities: a fixed-seed draw strictly inside (0, 1), not squashed
    scores, whose saturated 0 / 1 would exercise the clamp instead of the launcher."""
    from allrank_amd import losses as E
    jobs = [("approxNDCGLoss", {}), ("listNet", {}),
            ("lambdaLoss", dict(weighing_scheme="lambdaRank_scheme", sigma=1.3, mu=7.0)),
            ("lambdaLoss", dict(weighing_scheme="ndcgLoss2PP_scheme", k=5, reduction="mean", reduction_log="natural", sigma=1.3, mu=7.0)),
            ("neuralNDCG", dict(temperature=1.0)), ("neuralNDCG_transposed", dict(temperature=0.1, k=5)),
            ("listMLE", {}), ("rankNet", {}), ("rankNet_weightByGTDiff", {}), ("rankNet_weightByGTDiff_pow", {}), ("binary_listNet", {}),
            ("bce", {}), ("ordinal", dict(n=4)), ("pointwise_rmse", dict(no_of_levels=4))]
    seen = set()
    for st in ("main", "outlier"):
        B, L = SETS[st]
        g = torch.Generator().manual_seed(1000 * scale + L)
        perm = torch.randperm(L, generator=g)
        prob = (0.02 + 0.96 * torch.rand((B, L, 4), generator=g)).numpy()
        assert prob.min() > 0.0 and prob.max() < 1.0
        for name, kw in jobs:
            s, y = scale_golden["%s.x%d.s" % (st, scale)], scale_golden[st + ".y"]
            if name in ("bce", "ordinal", "pointwise_rmse"):
                s = prob if name == "ordinal" else np.ascontiguousarray(prob[:, :, 0])
            if name in ("bce", "binary_listNet"):
                y = scale_golden[st + ".yb"]
            fl = E.FusedLoss(name, B, L, "cuda:0", **kw)
            pkw = dict(kw)
            if name == "listMLE":
                fl.set_perm(perm)
                pkw["perm"] = perm
            loss, grad = fl.run(_t(s), _t(y), float(B))
            sp = _t(s, True)
            l2 = getattr(E, name)(sp, _t(y), **pkw)
            l2.backward()
            print("fused-vs-plugin", st, scale, name, float(loss), float(l2), float((grad - sp.grad).abs().max()))
            assert grad.shape == sp.grad.shape and torch.isfinite(grad).all(), (st, name)
            assert torch.equal(loss.reshape(()), l2.detach().reshape(())) and torch.equal(grad, sp.grad), (st, name, kw)
            seen.add(name)
    assert seen == set(E._LOSSES)                              # every name FusedLoss accepts


@pytest.mark.parametrize("scale", SCALES)
def test_metrics_match_reference_at_score_scale(scale, scale_golden):
    from allrank_amd import metrics as EM
    g = scale_golden
    for name, B, L, seed, ties, full in SCALE_SETS:
        pre = "%s.x%d." % (name, scale)
        s, y = g[pre + "s"], g[name + ".y"]
        ats = list(SCALE_NDCG_ATS) + [L]
        nd, order = EM.ndcg(_t(s), _t(y), ats=ats, return_order=True)
        dc = EM.dcg(_t(s), _t(y), ats=ats)
        assert close(nd.cpu().numpy(), g[pre + "ndcg"]) and close(dc.cpu().numpy(), g[pre + "dcg"]), pre
        order = order.cpu().numpy()
        nv = (y != -1).sum(1)
        for b in range(B):
            assert np.array_equal(order[b, :nv[b]], g[pre + "order"][b, :nv[b]]), (pre, b)      # bit-exact (tie policy)
        assert np.array_equal(EM.mrr(_t(s), _t(y), ats=list(SCALE_MRR_ATS)).cpu().numpy(), g[pre + "mrr"]), pre
