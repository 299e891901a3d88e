"""tests/metric_ref.py on the CPU (no GPU): (a) on every case the fp32 transcription of the NDCG / MRR kernels' arithmetic, in the kernels'
operation order, is inside every bar and equal in every exact output, so the bars are attainable; (b) every defect model is outside a bar,
or fails an exact output, on at least one case it applies to; (c) the references are oracle/ltr_oracle.py's in fp64 on the padded grid;
(d) the restated thread counts, LDS sizes, opt-in thresholds and limits are the sources', and EXPECTED_ARMS is what they give."""
import numpy as np
import pytest

from oracle import ltr_oracle as O
from tests import metric_ref as R
from tests.ragged_cases import grids, to_packed

GROUPS = sorted({(c.entry, c.L) for c in R.CASES})


def _caught(c, got):
    return any(R.over(*t).any() for t in R.checks(c, got).values()) or not R.exact_ok(c, got)


@pytest.mark.parametrize("entry,L", [pytest.param(*g, id="%s L %d" % g) for g in GROUPS])
def test_transcription_inside_every_bar_and_exact_where_the_kernel_is(entry, L):
    worst = {}
    for c in [c for c in R.CASES if (c.entry, c.L) == (entry, L)]:
        ref = R.reference(c)
        assert all(np.isfinite(ref[k]).all() for k in ref if k.startswith("bar_")), c.name
        assert (R.threads(entry, L), R.opts_in(entry, L)) == R.EXPECTED_ARMS.get((entry, L), (R.threads(entry, L), R.opts_in(entry, L))), c.name
        got = R.transcription(c)
        assert R.exact_ok(c, got), "%s: an exact output (order, filler, best_val / best_idx, the MRR bits) differs" % c.name
        for k, t in R.checks(c, got).items():
            worst[k] = max(worst.get(k, 0.0), R.worst(*t))
            assert not R.over(*t).any(), "%s: the transcription's %s is outside its bar, worst error / bar %.4g" % (c.name, k, R.worst(*t))
    print("%s L %d: worst error / bar  %s" % (entry, L, "  ".join("%s %.3g" % kv for kv in sorted(worst.items()))))


@pytest.mark.parametrize("family", ["ndcg", "mrr"])
def test_every_defect_is_outside_a_bar_or_fails_an_exact_output(family):
    entries = R.NDCG_ENTRIES if family == "ndcg" else R.MRR_ENTRIES
    cases = [c for c in R.CASES if c.entry in entries and c.L <= 3073]
    for wrong in (R.NDCG_WRONG if family == "ndcg" else R.MRR_WRONG):
        n = caught = 0
        for c in cases:
            if R.applies(c, wrong) is not None:
                continue
            n, caught = n + 1, caught + _caught(c, R.transcription(c, wrong))
        print("%s %-34s applies to %3d cases, told on %3d" % (family, wrong, n, caught))
        assert n > 0, "the defect %r applies to no case" % wrong
        assert caught > 0, "the defect %r is inside every bar and every exact output on every case" % wrong


def _same(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert (np.abs(a - b) <= 1e-12 * np.maximum(np.abs(b), 1e-300)).all(), what


def test_references_are_the_oracles():
    n = 0
    for c in R.CASES:
        i, ref = R.inputs(c), R.reference(c)
        bt = i.bt
        if c.L > 513 or c.order == "repeat" or c.draw in ("signed item gains", "wide item gains"):
            continue                                               # (per-item gains are no function of the label: the oracle has no form for them)
        if bt.ragged:
            s, y = grids(bt.s, bt.y, bt.cu, c.L)
            pack = lambda o: to_packed(o, bt.cu)                   # noqa: E731
        else:
            s, y, pack = bt.s.astype(np.float64), bt.y.astype(np.float64), lambda o: o     # noqa: E731
        if R.is_mrr(c):
            _same(ref["mrr"], O.mrr(s, y, ats=list(c.ats), dtype=np.float64), c.name)
        else:
            fn = (lambda t: t + 1) if c.draw == "gain y+1" else None
            with np.errstate(all="ignore"):
                nd, order = O.ndcg(s, y, ats=list(c.ats), filler_value=float(R.FILLER), dtype=np.float64, gain_function=fn)
                dc, _ = O.dcg(s, y, ats=list(c.ats), dtype=np.float64, gain_function=fn)
            _same(ref["ndcg"], nd, c.name + " ndcg"), _same(ref["dcg"], dc, c.name + " dcg")
            assert np.array_equal(ref["order"], pack(order)), c.name
        n += 1
    assert n >= 40


def test_restated_constants_and_thresholds_are_the_sources():
    k = R.source_constants()
    assert k["ndcg_block"] == (256, 512, 1024, 256) and k["ndcg_lds"] == ["4"] and k["mrr_launch"] == [("256", "2"), ("256", "2")]
    assert k["default_lds"] == R.DEFAULT_DYN_LDS and k["max_ats"] == R.MAX_ATS and k["max_metric_l"] == R.MAX_METRIC_L
    for (entry, L), arm in R.EXPECTED_ARMS.items():
        assert (R.threads(entry, L), R.opts_in(entry, L)) == arm, (entry, L)
    assert [R.threads("ltrx_ndcg_at", L) for L in (512, 513)] == [256, 1024] and [R.threads("ltrx_ndcg_at_cu", L) for L in (256, 257)] == [256, 1024]
    assert [R.opts_in("ltrx_ndcg_at", L) for L in (3072, 3073)] == [False, True] and [R.opts_in("ltrx_mrr_at", L) for L in (6144, 6145)] == [False, True]
    assert R.lds_bytes("ltrx_mrr_at", R.MAX_METRIC_L) == 64 * 1024 and R.lds_bytes("ltrx_ndcg_at", R.MAX_METRIC_L) == 128 * 1024


def test_the_table_reaches_every_length_switch_and_option():
    by = lambda **kw: [c for c in R.CASES if all(getattr(c, k) == v for k, v in kw.items())]      # noqa: E731
    assert {c.L for c in by(entry="ltrx_ndcg_at")} == set(R.PADDED_L)
    assert {c.L for c in by(entry="ltrx_mrr_at")} == set(R.PADDED_L) | set(R.MRR_EXTRA_L)
    for entry in ("ltrx_ndcg_at", "ltrx_mrr_at", "ltrx_ndcg_at_cu", "ltrx_mrr_at_cu"):
        assert {len(c.ats) for c in by(entry=entry)} >= {1, 3, 16} or entry.endswith("_cu"), entry
        assert {(R.threads(entry, c.L), R.opts_in(entry, c.L)) for c in by(entry=entry)} == {a for (e, _), a in R.EXPECTED_ARMS.items() if e == entry}, entry
    assert {c.order for c in by(entry="ltrx_ndcg_at_cu")} == {None, "perm", "longest", "repeat"}
    assert {c.order for c in by(entry="ltrx_mrr_at_cu")} == {None, "perm", "longest", "repeat"}
    assert {c.L for c in by(entry="ltrx_ndcg_at_cu")} == {256, 257, 3073}
    for c in R.CASES:
        bt = R.inputs(c).bt
        assert 1 in c.ats or len(c.ats) == 1 or c.draw == "wide item gains", c.name
        assert max(c.ats) > c.L or len(c.ats) == 1, c.name
        if bt.ragged:
            n = np.diff(bt.cu)
            assert 0 in n and 1 in n and n.max() == c.L, c.name
            if c.L == 257:
                assert tuple(n) == R.RAGGED_LENGTHS
            if c.order == "repeat":
                assert not R.visited(bt).all() and R.visited(bt).sum() == bt.B - 2
            elif c.order is not None:
                assert sorted(bt.order.tolist()) == list(range(bt.B)) and (c.order != "longest" or n[bt.order[0]] == c.L)
        else:
            nv = (bt.y != R.PAD).sum(1)
            assert nv[0] == c.L and (c.L >= 3072 or (nv[1] == 1 and nv[2] == 0 and not bt.y[4].any())), c.name
    sg = [c for c in R.CASES if c.draw == "signed item gains"][0]
    assert (R.inputs(sg).gains < 0).any() and not R.reference(sg)["filler"].any()
