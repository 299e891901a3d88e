"""No GPU: ``ragged.form_of`` over every loss of allrank_amd.losses, and the property that makes the ragged contract well defined --
the fp64 oracle gives the same value on the padded grid whatever its width, so "the padded call on any grid of width >= max_len"
names ONE number.  The expectations of tests/test_gpu_ragged.py are the width-257 values checked here."""
import functools

import numpy as np
import pytest

from tests import ragged_cases as RC

# fp64 on grids of two widths: identical terms, but numpy's pairwise sums group them differently.  Each sum of n <= 921^2 terms is then
# off by at most about log2(n) * 2^-53 ~ 2e-15 of the sum of the terms' magnitudes; the bar leaves three decimal orders above that.
RTOL = 1e-12


def _same(a, b, scale=None):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    nan = np.isnan(a) & np.isnan(b)
    mag = np.abs(b).max() if scale is None and b.size else (scale or 0.0)
    return bool(np.all(nan | (np.abs(a - b) <= RTOL * max(float(mag), 1e-300))))


def test_form_of_covers_every_loss_and_keeps_the_bound_arguments():
    from allrank_amd import losses as E, metrics as EM, ragged
    covered = {"listNet": ragged.listNet, "approxNDCGLoss": ragged.approxNDCGLoss, "lambdaLoss": ragged.lambdaLoss}
    plain = [n for n in E.__all__ if callable(getattr(E, n)) and n not in ("sinkhorn_iterations_used", "with_ordinals")]
    assert set(E._LOSSES) <= set(plain)
    for name in plain:
        fn = getattr(E, name)
        assert ragged.form_of(fn) is covered.get(name), name
        assert (ragged.form_of(functools.partial(fn)) is not None) == (name in covered), name
    # the bound keyword arguments survive; the padding value, which the layout does not have, is dropped
    f = ragged.form_of(functools.partial(E.lambdaLoss, weighing_scheme="ndcgLoss2PP_scheme", k=5, mu=7.0, reduction="mean",
                                         padded_value_indicator=-1))
    assert f.func is ragged.lambdaLoss and f.keywords == dict(weighing_scheme="ndcgLoss2PP_scheme", k=5, mu=7.0, reduction="mean")
    f = ragged.form_of(functools.partial(E.approxNDCGLoss, alpha=2.5, eps=1e-9))
    assert f.func is ragged.approxNDCGLoss and f.keywords == dict(alpha=2.5, eps=1e-9)
    assert ragged.form_of(functools.partial(E.listNet, padded_value_indicator=-1)) is ragged.listNet
    # no ragged form
    assert ragged.form_of(functools.partial(E.listMLE, eps=1e-9)) is None
    assert ragged.form_of(functools.partial(E.neuralNDCG, stochastic=True)) is None
    assert ragged.form_of(functools.partial(E.ordinal, n=4)) is None
    assert ragged.form_of(functools.partial(E.listNet, 1.0)) is None                 # positionally bound
    assert ragged.form_of(lambda a, b: a) is None and ragged.form_of(None) is None and ragged.form_of([]) is None
    # the metrics, and a custom gain function
    assert ragged.form_of(EM.ndcg) is ragged.ndcg and ragged.form_of(EM.dcg) is ragged.dcg and ragged.form_of(EM.mrr) is ragged.mrr
    assert ragged.form_of(functools.partial(EM.ndcg, gain_function=lambda x: x)) is None
    assert ragged.form_of(functools.partial(EM.ndcg, ats=[5], padding_indicator=-1)).keywords == dict(ats=[5])


def test_ragged_signatures_are_the_padded_ones_without_the_padding_value():
    import inspect
    from allrank_amd import losses as E, metrics as EM, ragged
    lead = ["y_pred", "y_true", "cu_seqlens", "max_len", "slate_order"]
    for pad_fn, rag_fn in ((E.listNet, ragged.listNet), (E.approxNDCGLoss, ragged.approxNDCGLoss), (E.lambdaLoss, ragged.lambdaLoss),
                           (EM.ndcg, ragged.ndcg), (EM.dcg, ragged.dcg), (EM.mrr, ragged.mrr)):
        pp, rp = inspect.signature(pad_fn).parameters, inspect.signature(rag_fn).parameters
        assert list(rp)[:5] == lead, rag_fn.__name__
        want = [k for k in list(pp)[2:] if k not in ("padded_value_indicator", "padding_indicator")]
        assert list(rp)[5:] == want, rag_fn.__name__
        assert all(rp[k].default == pp[k].default for k in want), rag_fn.__name__
        assert rp["max_len"].default is None and rp["slate_order"].default is None


@pytest.fixture(scope="module")
def two_widths():
    """scale -> [(padded scores, padded labels, cu) at each width]"""
    out = {}
    for scale in (1, 30):
        s, y, cu = RC.make_batch(scale)
        out[scale] = [RC.grids(s, y, cu, L) + (cu,) for L in RC.PAD_WIDTHS]
    return out


def test_the_batch_has_the_properties_the_gpu_tests_rely_on():
    s, y, cu = RC.make_batch(1)
    lens = np.diff(cu)
    assert tuple(lens) == RC.LENGTHS and cu.dtype == np.int32 and s.dtype == y.dtype == np.float32 and len(s) == cu[-1] == sum(RC.LENGTHS)
    assert set(np.unique(y)) == {0.0, 1.0, 2.0, 3.0, 4.0}
    b = RC.ZERO_LABEL_SLATE
    assert lens[b] == 31 and not y[cu[b]:cu[b + 1]].any()
    for b in range(len(lens)):
        sl = s[cu[b]:cu[b + 1]]
        if lens[b] >= 2:
            assert len(np.unique(sl)) < len(sl), b                     # an exact tie in the scores of every slate of 2+ items
        if lens[b] >= 31 and b != RC.ZERO_LABEL_SLATE:
            assert len(np.unique(y[cu[b]:cu[b + 1]])) < lens[b]        # ties in the labels
    assert np.array_equal(RC.make_batch(30)[0], s * np.float32(30))


@pytest.mark.parametrize("scale", [1, 30])
def test_listnet_and_approxndcg_do_not_depend_on_the_pad_width(scale, two_widths):
    (a, b) = two_widths[scale]
    for fn in (RC.listnet_expected, RC.approxndcg_expected):
        la, ga, pa = fn(*a)
        lb, gb, pb = fn(*b)
        assert np.isfinite(la) and np.isfinite(ga).all() and np.isfinite(pa).all(), fn.__name__
        assert _same(la, lb) and _same(ga, gb) and _same(pa, pb), fn.__name__
        assert pa[0] == 0.0                                            # the empty slate contributes nothing


@pytest.mark.parametrize("scale", [1, 30])
def test_lambdaloss_does_not_depend_on_the_pad_width(scale, two_widths):
    """the whole case matrix at scale 1; at scale 30 the untruncated 'sum' case of every scheme (the width-921 oracle dominates the
    time of this file)"""
    (a, b) = two_widths[scale]
    for c in RC.LAMBDA_CASES:
        if scale != 1 and (c[1] is not None or c[2] != "sum"):
            continue
        la, ga, na, oa = RC.lambdaloss_expected(*a, *c)
        lb, gb, nb, ob = RC.lambdaloss_expected(*b, *c)
        assert na == nb and na > 0 and np.array_equal(oa, ob), c
        assert np.isfinite(la) and _same(la, lb) and _same(ga, gb), c


@pytest.mark.parametrize("scale", [1, 30])
def test_metrics_do_not_depend_on_the_pad_width(scale, two_widths):
    (a, b) = two_widths[scale]
    nda, dca, oa, mra = RC.metrics_expected(*a, filler=0.25)
    ndb, dcb, ob, mrb = RC.metrics_expected(*b, filler=0.25)
    assert _same(nda, ndb) and _same(dca, dcb) and np.array_equal(oa, ob) and np.array_equal(mra, mrb)
    assert np.all(nda[0] == 0.25) and np.all(nda[RC.ZERO_LABEL_SLATE] == 0.25) and not dca[0].any()      # filler: empty and zero-label slates
    # an empty slate's first maximum is (label 0, rank 0), as a fully padded slate's: reciprocal rank 1 unless the batch rule zeroes it
    assert np.all(mra[0] == 1.0) and np.all(mra[RC.ZERO_LABEL_SLATE] == 1.0)
    # in-slate order: a permutation of every slate's own indices
    cu = a[2]
    for s in range(len(cu) - 1):
        assert sorted(oa[cu[s]:cu[s + 1]]) == list(range(cu[s + 1] - cu[s]))
    # a batch of zero labels: the reference's batch-level rule zeroes every entry
    z = RC.metrics_expected(a[0], np.where(a[1] == -1, -1.0, 0.0), cu)[3]
    assert not z.any()
