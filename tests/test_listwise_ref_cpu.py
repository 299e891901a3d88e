"""tests/listwise_ref.py on the CPU (no GPU): (a) on every case up to L = 1025 the fp32 transcription of the kernels' arithmetic, in the
kernels' operation order, is inside every bar, so the bars are attainable, and the branch guard holds on every case (the long ones need
the reference only); (b) every defect model is outside a bar, or fails an exact output, on at least one case it applies to; (c) the
references are oracle/ltr_oracle.py's in fp64; (d) the restated array counts, budgets, block sizes and thresholds are the sources'.

For each defect the test also records whether the bar the suite had until now -- tests.cases.grad_close(rtol=2e-4) on the gradient and
tests.cases.close on the loss -- would have told it on the same cases, and counts the floating-point bars (gradient, per-slate, loss)
apart from the exact outputs (order_out, the pair count, padded zeros), which the suite compared exactly before.
MISSED_BY_THE_MAX_NORM_BAR lists the defects for which, on at least one case, the max-norm bar passes and a FLOATING-POINT entrywise bar
fails; the assertion keeps the list honest:
    lq_rounded_down (lambdaLoss, approxNDCG)   lq = n >> 2: the n % 4 last items are nobody's partner.  Where the last item stands before
                                        nobody in either ranking (label 0, the lowest score: the "low tail" cases) every rank is
                                        unchanged, order_out with it, and the pairs it drops are near saturation: small against the
                                        slate's largest entry, far outside the entries' own bars
    quarter_tail_dropped (lambdaLoss)   every quarter one partner short: two cases of the table
    discount_at_rank (lambdaLoss)       1 / log2(1 + rank) for 1 / log2(2 + rank) in maxDCG; with a cut and a saturated slate the entries
                                        that move are small against the largest
    rj_gt_kk (lambdaLoss)               the cut one above the last rank at score scale 30: the item it wrongly admits is far below every
                                        partner, 1 - sigmoid is tiny, and only the entries of its neighbours move
    clamp_c_not_zeroed (approxNDCG), scan_base_by_subtraction (ListMLE: the kernel's own code until this table existed)
In lambdaLoss a lost or added partner is a lost or added selected pair, so the exact pair count (and, where ranks move, order_out),
which tests/test_gpu_ragged.py and tests/test_gpu_parity.py compared exactly before, tells the two dropped-partner defects and rj_gt_kk
on those cases too; NOTHING_ELSE_TELLS are the defects with a case where the max-norm bar passes, every exact output is equal and a
floating-point bar fails -- approxNDCG, which has no exact output, carries the dropped partner there.  tie_reversed and padded_counted of
lambdaLoss are not on the list: wherever the max-norm bar passes them no floating-point bar fails, and order_out alone tells them."""
import numpy as np
import pytest

from oracle import ltr_oracle as O
from tests import listwise_ref as R
from tests.cases import close, grad_close

MISSED_BY_THE_MAX_NORM_BAR = {"lambdaloss": ("quarter_tail_dropped", "lq_rounded_down", "discount_at_rank", "rj_gt_kk"), "approxndcg": ("lq_rounded_down", "clamp_c_not_zeroed"),
                              "listmle": ("scan_base_by_subtraction",), "listnet": ()}
NOTHING_ELSE_TELLS = {("approxndcg", "lq_rounded_down"), ("approxndcg", "clamp_c_not_zeroed"), ("lambdaloss", "discount_at_rank"),
                      ("listmle", "scan_base_by_subtraction")}      # max-norm bar passes, every exact output equal, a floating-point bar fails
ORDER_ONLY = {"lambdaloss": ("tie_reversed", "padded_counted")}
GROUPS = sorted({(c.loss, c.layout, c.L) for c in R.CASES})


def _fp_caught(c, got):
    """a floating-point output (gradient, per-slate value, loss) is outside its bar"""
    return any(R.over(*t).any() for t in R.checks(c, got).values())


def _caught(c, got):
    return _fp_caught(c, got) or not R.exact_ok(c, got)


def _old_bar_passes(c, got):
    ref = R.reference(c)
    return grad_close(got["grad"], ref["grad"]) and close(got["loss"], ref["loss"])


@pytest.mark.parametrize("loss,layout,L", [pytest.param(*g, id="%s %s L %d" % g) for g in GROUPS])
def test_transcription_inside_every_bar_and_the_branch_guard_holds(loss, layout, L):
    worst = {}
    for c in [c for c in R.CASES if (c.loss, c.layout, c.L) == (loss, layout, L)]:
        ref = R.reference(c)                                   # asserts the guard: no clamp decision inside its band
        assert not ref.get("violations")
        assert c.long == (c.L > R.MAX_F32_L) and c.arm == R.EXPECTED_ARMS.get((c.loss, c.L), c.arm)
        assert np.isfinite(ref["bar_grad"]).all() and np.isfinite(ref["grad"]).all()
        if c.long:
            continue
        got = R.transcription(c)
        assert R.exact_ok(c, got), "%s: an exact output (padded zeros, pair count, order) differs" % c.name
        for k, t in R.checks(c, got).items():
            worst[k] = max(worst.get(k, 0.0), R.worst(*t))
            assert not R.over(*t).any(), "%s: the transcription's %s is outside its bar, worst error / bar %.4g" % (c.name, k, R.worst(*t))
    print("%s %s L %d: worst error / bar  %s" % (loss, layout, L, "  ".join("%s %.3g" % kv for kv in sorted(worst.items()))))


def _defect_cases(loss):
    """every case up to L = 257 (listMLE: 512, its last length with two items per scan thread); of lambdaLoss's full matrix every fourth
    configuration per length and scale (the stride walks every scheme, cut and reduction over the lengths), and every extra case"""
    out = []
    for i, c in enumerate(R.CASES):
        if c.loss != loss or c.L > (512 if loss == "listmle" else 257):
            continue
        if loss == "lambdaloss" and c.layout == "padded" and c.par.ext is None and not c.low_tail and c.par.k != c.L - 1 and i % 4:
            continue
        out.append(c)
    return out


@pytest.mark.parametrize("loss", sorted(R.WRONG))
def test_every_defect_is_outside_a_bar_and_which_the_max_norm_bar_missed(loss):
    cases = _defect_cases(loss)
    missed_by_old = []
    for wrong in R.WRONG[loss]:
        n = caught = fp = old = fp_alone = exact_alone = clean = 0
        for c in cases:
            if R.applies(c, wrong) is not None:
                continue
            bad = R.transcription(c, wrong)
            f, x, o = _fp_caught(c, bad), not R.exact_ok(c, bad), not _old_bar_passes(c, bad)
            n, caught, fp, old = n + 1, caught + (f or x), fp + f, old + o
            fp_alone, exact_alone, clean = fp_alone + (f and not o), exact_alone + (x and not f and not o), clean + (f and not o and not x)
        print("%s %-26s applies to %3d cases; outside a floating-point bar on %3d, that or an exact output on %3d; outside the max-norm bar on "
              "%3d; a floating-point bar alone %3d (with every exact output equal %3d), an exact output alone %3d" % (
                  loss, wrong, n, fp, caught, old, fp_alone, clean, exact_alone))
        assert n > 0, "%s: the defect %r applies to no case" % (loss, wrong)
        assert caught > 0, "%s: the defect %r is inside every bar on every case" % (loss, wrong)
        if fp_alone:
            missed_by_old.append(wrong)
        if (loss, wrong) in NOTHING_ELSE_TELLS:
            assert clean > 0, (loss, wrong)
        if wrong in ORDER_ONLY.get(loss, ()):
            assert exact_alone > fp_alone, (loss, wrong, n, caught, fp_alone, exact_alone)
    assert set(MISSED_BY_THE_MAX_NORM_BAR[loss]) <= set(missed_by_old), (loss, missed_by_old)


def test_the_switches_of_approxndcg_that_are_no_defects_change_nothing():
    """padded_counted and clamp_a_not_zeroed change no bit; a tie broken the other way hands the same ranks to other threads, so maxDCG is
    summed in another order: the same value, inside every bar"""
    for c in [c for c in R.CASES if c.loss == "approxndcg" and c.L <= 257]:
        good = R.transcription(c)
        for same in R.APPROX_SAME:
            other = R.transcription(c, same)
            if same == "tie_reversed":
                assert not _caught(c, other), (c.name, same)
                continue
            assert all(np.array_equal(np.asarray(good[k], np.float32).view(np.uint32), np.asarray(other[k], np.float32).view(np.uint32))
                       for k in ("loss", "per", "grad")), (c.name, same)


def _k(p):
    return None if p.k <= 0 else p.k


@pytest.mark.parametrize("loss", sorted(R.WRONG))
def test_references_are_the_oracles(loss):
    """the padded cases at score scale 1 up to L = 257 (for lambdaLoss: every scheme, cut and reduction of the matrix at L = 5 and every
    fourth at L = 257) against oracle/ltr_oracle.py with dtype=np.float64 and the widened fp32 parameters"""
    eps = R.w(R.EPS)
    n = 0
    for i, c in enumerate(R.CASES):
        if c.loss != loss or c.layout != "padded" or c.scale != 1 or c.L > 257 or (loss == "lambdaloss" and c.L > 5 and i % 4):
            continue
        bt, ref = R.inputs(c), R.reference(c)
        s, y = bt.s.astype(np.float64), bt.y.astype(np.float64)
        with np.errstate(all="ignore"):
            if loss == "listnet":
                _, grad, per = O.listnet(s, y, eps=eps, dtype=np.float64)
                empty = ~(bt.y != R.PAD).any(1)
                per, grad = np.where(empty, 0.0, per), np.nan_to_num(grad)
                out = dict(loss=per.sum() / bt.B, grad=grad, per=per)
            elif loss == "listmle":
                l, grad, per, order = O.listmle(s, y, R.perm_of(c), eps=eps, dtype=np.float64)
                out = dict(loss=l, grad=grad, per=per)
                assert np.array_equal(order, ref["order"]), c.name
            elif loss == "approxndcg":
                l, grad, per = O.approxndcg(s, y, eps=eps, alpha=R.w(c.par), dtype=np.float64)
                out = dict(loss=l, grad=grad, per=per)
            else:
                p = c.par
                if p.ext is not None:
                    continue
                l, grad, n_sel, ip = O.lambdaloss(s, y, eps=eps, weighing_scheme=R.SCHEMES[p.scheme], k=_k(p), sigma=R.w(p.sigma), mu=R.w(p.mu),
                                                  reduction="mean" if p.mean else "sum", reduction_log="natural" if p.natural else "binary",
                                                  dtype=np.float64)
                out = dict(loss=l, grad=grad)
                assert n_sel == ref["count"] and np.array_equal(ip, ref["order"]), c.name
        for k, v in out.items():
            a, b = np.asarray(ref[k], np.float64), np.asarray(v, np.float64)
            both_nan = np.isnan(a) & np.isnan(b)
            top = float(np.abs(np.nan_to_num(b)).max()) if b.size else 0.0
            assert (both_nan | (np.abs(a - b) <= 1e-10 * max(top, 1e-300))).all(), (c.name, k)
        n += 1
    assert n >= 8


def test_restated_constants_and_thresholds_are_the_sources():
    k = R.source_constants()
    assert k["narr"] == R.NARR and k["budget"] == R.LDS_BUDGET and k["default_lds"] == R.DEFAULT_DYN_LDS and k["max_long"] == R.MAX_LONG
    assert k["threads"] == dict(listmle=(512, 1024, 256), listnet=["256"], approxndcg=["1024"], lambdaloss=["1024"])
    assert [R.block_threads("listmle", L) for L in (512, 513)] == [256, 1024] and R.block_threads("lambdaloss", 1) == 1024
    # the array counts 2 / 6 / 7 / 13 (+ 2) give the lengths the issue of this table names
    assert R.thresholds("lambdaloss") == (945, 946, 3130, 3131) and R.thresholds("approxndcg") == (1755, 1756, 5814, 5815)
    assert R.thresholds("listmle") == (2048, 2049, 6784, 6785) and R.thresholds("listnet") == (6144, 6145)
    assert R.in_lds("listnet", R.MAX_LONG), "listNet has a reachable workspace arm now: the table needs its cases"
    for loss in R.NARR:
        a, b = R.last_lds(loss, R.DEFAULT_DYN_LDS), R.last_lds(loss)
        assert not R.opts_in(loss, a) and R.opts_in(loss, a + 1) and R.in_lds(loss, b) and not R.in_lds(loss, b + 1)
        assert R.workspace_bytes(loss, 3, a) == R.per_floats(loss, 3) * 4
    assert R.workspace_bytes("lambdaloss", 3, 3131) == (12 + 3 * ((13 * 3131 + 2 + 3) & ~3)) * 4
    assert R.workspace_bytes("approxndcg", 3, 5815) == (4 + 3 * ((7 * 5815 + 3) & ~3)) * 4


def test_the_table_reaches_every_arm_length_and_option():
    by = lambda **kw: [c for c in R.CASES if all(getattr(c, k) == v for k, v in kw.items())]      # noqa: E731
    for loss in R.NARR:
        lengths = {c.L for c in by(loss=loss, layout="padded")}
        assert set(R.SHORT) | set(R.thresholds(loss)) <= lengths, loss
        assert {c.scale for c in by(loss=loss) if c.L <= 257} == {1, 30} and {c.scale for c in by(loss=loss) if c.L > 512} == {1}
        arms = {c.arm for c in by(loss=loss, layout="padded")}
        assert arms == ({"LDS", "LDS opt-in"} if loss == "listnet" else {"LDS", "LDS opt-in", "GWS"}), (loss, arms)
    assert set(R.KILO) <= {c.L for c in by(loss="lambdaloss")} & {c.L for c in by(loss="approxndcg")} & {c.L for c in by(loss="listmle")}
    lam = by(loss="lambdaloss", layout="padded")
    for L in R.SHORT:
        for scale in (1, 30):
            assert {(c.par.scheme, c.par.k, c.par.mean) for c in lam if c.L == L and c.scale == scale} >= {
                (sc, k, m) for sc in range(8) for k in (0, 5, L, L + 3) for m in (False, True)}, (L, scale)
    assert set(R.EXPECTED_ARMS) >= {(loss, L) for loss in R.NARR for L in R.thresholds(loss)}
    assert any(c.low_tail for c in by(loss="approxndcg")) and any(c.low_tail for c in lam)
    assert {c.par.scheme for c in lam if c.arm == "GWS"} == {3, 4} and any(c.par.ext is not None for c in lam)
    assert {c.par for c in by(loss="approxndcg", layout="padded")} == {1.0, 2.5} and {c.par for c in by(loss="listmle")} == {"identity", "seeded"}
    for loss in ("listnet", "approxndcg", "lambdaloss"):
        assert {c.order for c in by(loss=loss, layout="ragged", L=257)} == {False, True}
    assert [c.arm for c in by(layout="ragged") if c.L > 257] == ["GWS"] * 3
    for c in R.CASES:
        bt = R.inputs(c)
        if c.layout == "padded":
            nv = (bt.y != R.PAD).sum(1)
            assert (len(set(nv.tolist())) == bt.B or c.L < 5) and (bt.B == 3) == (c.arm == "GWS" or c.long), c.name
            if bt.B == 4:
                assert nv[2] == 0 and not bt.y[1][bt.y[1] != R.PAD].any()                  # fully padded; all labels 0
            if c.L >= 2:
                tie = c.L - 2 if c.low_tail and c.L >= 3 else c.L - 1
                assert bt.s[0, 0] == bt.s[0, tie]                                          # an exact tie
            if c.low_tail:
                assert bt.s[0, -1] < bt.s[0, :-1].min() - 0.9 * R.LOW_TAIL_GAP and bt.y[0, -1] == 0
        else:
            assert 0 in np.diff(bt.cu) and 1 in np.diff(bt.cu) and np.diff(bt.cu).max() == c.L
