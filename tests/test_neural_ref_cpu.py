"""The evidence that the NeuralNDCG contract of tests/neural_ref.py bites, without a GPU: the fp32 transcriptions are inside every bar on
every case (the reference formulation in three summation orders within bar / 4: that is how K was measured), every defect model is outside
on its named case, the derived tolerances give the same exit step in fp32 and fp64, the fp64 reference agrees with oracle/ltr_oracle.py,
and the plain and transposed formulas agree on the valid block.  test_defects_the_max_norm_bar_lets_through prints what
tests.cases.grad_close at rtol = 5e-4 (the bar of test_gpu_parity.py) cannot see."""
import os
import re

import numpy as np
import pytest

from oracle import ltr_oracle as O
from tests import neural_ref as R
from tests.cases import grad_close

OUTPUTS = ("grad", "per", "loss", "idcg")


def _ratios(got, ref):
    return {k: R.worst(*v) for k, v in R.checks(got, ref).items()}


def test_restated_constants_match_the_source():
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "allrank_amd", "csrc", "ltrx_neuralndcg.hip")
    src = open(here).read()
    assert re.search(r"const bool blk = \(L <= (\d+)\) && path == 0;", src).group(1) == str(R.BLOCK_MAX_L)
    fwd = re.findall(r"if \(L <= (\d+)\) LTRX_NEURAL_FWD_BLK\(\d+, (\d+), (\d+), \d+\);", src)
    bwd = re.findall(r"if \(L <= (\d+)\) LTRX_NEURAL_BWD_BLK\(\d+, (\d+), (\d+), \d+, \d+\);", src)
    assert fwd == bwd == [(str(top), str(wd), str(wd)) for top, _, wd in R.GEOMETRIES[:3]]
    assert "else LTRX_NEURAL_FWD_BLK(4, 15, 5, 3);" in src and "else LTRX_NEURAL_BWD_BLK(4, 15, 5, 3, 2);" in src
    assert "constexpr float kSinkEps = 1e-10f;" in src
    assert ("return align64((size_t)B * 4) + align64((size_t)B * mi * 4) + 64 + align64((size_t)B * (mi + 1) * L * 4) +\n"
            "         align64((size_t)B * mi * L * 4) + 2 * align64((size_t)B * L * L * 4) + 64;") in src
    hdr = open(os.path.join(os.path.dirname(here), "..", "..", "include", "ltrx.h")).read()
    assert int(re.search(r"#define LTRX_MAX_SLATE_LEN (\d+)", hdr).group(1)) == R.MAX_SLATE_LEN
    assert float(re.search(r"#define LTRX_NEURALSORT_PAD \((-[0-9.e]+)f\)", hdr).group(1)) == R.NSORT_PAD
    for (path, L), arm in R.EXPECTED_ARMS.items():
        assert R.arm_of(path, L) == arm


def test_case_table_covers_what_it_names():
    names = [c.name for c in R.CASES]
    assert len(set(names)) == len(names)
    assert {c.L for c in R.CASES if c.path == 0} >= {1, 2, 3, 63, 64, 65, 128, 129, 192, 193, 240, 241, 257}
    assert {c.L for c in R.CASES if c.path == 1} >= {3, 64, 129, 240}
    assert {R.arm_of(c.path, c.L) for c in R.CASES if c.T is not None} == set(R.REWIND_ARMS), "a rewind on every arm"
    assert {c.tau for c in R.CASES} >= {0.1, 1.0, 10.0} and {c.powered for c in R.CASES} == {True, False}
    assert {c.transposed for c in R.CASES} == {True, False} and {c.max_iter for c in R.CASES} >= {0, 1, 50}
    assert any(c.k_rows for c in R.CASES) and {0, 1, 5} <= {c.k for c in R.CASES} and any(c.scale == 30 for c in R.CASES)
    for c in R.CASES:
        s, y = R.inputs(c)
        assert 2 <= len(c.counts) <= 5 and [int((row != R.PAD).sum()) for row in y] == list(c.counts)
        if c.k_rows:
            assert len(c.k_rows) == len(c.counts) and min(c.k_rows) < c.k
        if c.pad in ("inter", "clamp"):                        # some valid row sits at an original index >= n
            assert any(0 < n and np.flatnonzero(row != R.PAD).max() >= n for row, n in zip(y, c.counts))
    for top, arm, wd in R.GEOMETRIES:
        assert any(R.arm_of(c.path, c.L) == arm and any(n > wd and n % wd == 1 for n in c.counts) for c in R.CASES), arm
    exc = R.reference(R.case("L 3 path 0 all excluded"))
    assert exc["cnt"] == 0 and exc["loss"] == 0 and not exc["grad"].any() and not exc["per"].any()
    glob = R.case("L 64 path 0 batch-global exit")
    res = R.reference(glob)["res"]
    first = [int(np.flatnonzero(r < R.tol_of(glob))[0]) + 1 for r in res]
    assert first[0] == 1 and first[1] < first[2] == glob.T, first


@pytest.mark.parametrize("c", R.CASES, ids=lambda c: c.name)
def test_transcriptions_are_inside_the_bars(c):
    ref = R.reference(c)
    s, y = R.inputs(c)
    for order in R.ORDERS:
        got = R._core(s, y, R.par_of(c), R.tol_of(c), np.float32, order)
        assert got["T"] == ref["T"] and got["cnt"] == ref["cnt"], "%s (%s): T* %d, the fp64 reference has %d" % (c.name, order, got["T"], ref["T"])
        for k, r in _ratios(got, ref).items():
            assert r <= 1.0 / R.FACTOR, "%s: the reference formulation in fp32 (%s order) is at %.3g of the bar of %s" % (c.name, order, r, k)
    got = R.transcription(c)
    assert R.exact_ok(got, ref), "%s: the kernel-order transcription differs in an exact output (T* %d vs %d)" % (c.name, got["T"], ref["T"])
    for k, r in _ratios(got, ref).items():
        print("%s: kernel-order transcription %s error / bar %.3g" % (c.name, k, r))
        assert r <= 1.0, "%s: the kernel-order transcription is outside the bar of %s (%.3g)" % (c.name, k, r)


def test_K_is_the_measured_worst_times_the_factor():
    for k in OUTPUTS:
        assert R.K[k] == R.FACTOR * R.WORST[k]
    worst, _ = R.measure([c for c in R.CASES if c.L <= 65])                       # the whole table runs in the test above, within bar / FACTOR
    for k in OUTPUTS:
        assert worst[k] <= R.WORST[k]


@pytest.mark.parametrize("wrong", R.WRONG)
def test_every_defect_model_is_outside_on_its_named_case(wrong):
    c = R.case(R.NAMED[wrong])
    ref = R.reference(c)
    got = R.transcription(c, wrong)
    r = _ratios(got, ref)
    print("%s on %s: %s, exact outputs %s" % (wrong, c.name, " ".join("%s %.3g" % kv for kv in r.items()), R.exact_ok(got, ref)))
    assert max(r.values()) > 1.0 or not R.exact_ok(got, ref)
    if wrong not in ("residual_rows_only", "excluded_slate_counted", "gain_of_padded_not_zero"):      # those show in T*, the count, idcg
        assert max(r["grad"], r["per"]) > 1.0, "%s must show in the values or the gradient of %s" % (wrong, c.name)


def test_derived_tolerances_are_guarded_and_unambiguous():
    wanted = [c for c in R.CASES if c.T is not None]
    assert len(wanted) >= 5
    for c in wanted:
        tol = R.tol_of(c)                                                            # asserts the guard
        m = R.reference(c)["res"].max(0)
        assert 2 <= c.T < c.max_iter and m[c.T - 1] < tol < m[c.T - 2] and tol > R.GUARD * max(c.counts) * R.U
        s, y = R.inputs(c)
        for order in R.ORDERS:
            assert R._core(s, y, R.par_of(c), tol, np.float32, order)["T"] == c.T
        assert R.transcription(c)["T"] == c.T


def test_reference_agrees_with_the_oracle_in_fp64():
    for c in R.CASES:
        if c.k_rows is not None:
            continue
        ref = R.reference(c)
        s, y = R.inputs(c)
        loss, grad, n_iter = O.neuralndcg(s, y, temperature=R.w(c.tau), powered_relevancies=c.powered, k=None if c.k <= 0 else c.k, transposed=c.transposed,
                                          max_iter=c.max_iter, tol=R.tol_of(c), dtype=np.float64)
        # the reference clamps at the fp32 value of 1e-10 (what the kernels and torch's fp32 clamp see), the oracle in fp64 at 1e-10 itself:
        # 4e-9 apart, which shows only where a clamp is active
        rtol = 1e-7 if c.pad == "clamp" else 1e-11
        assert n_iter == ref["T"], c.name
        assert abs(loss - ref["loss"]) <= rtol * max(1.0, abs(ref["loss"])), c.name
        assert np.abs(grad - ref["grad"]).max() <= rtol * max(np.abs(ref["grad"]).max(), 1e-30), c.name


def test_plain_and_transposed_formulas_agree_for_matching_idcg():
    for c in R.CASES:
        s, y = R.inputs(c)
        p, tol = R.par_of(c), R.tol_of(c)
        a = R._core(s, y, p._replace(transposed=True), tol)
        b = R._core(s, y, p._replace(transposed=False), tol, idcg_given=a["idcg"])
        assert np.abs(a["per"] - b["per"]).max() <= 1e-13 and np.abs(a["grad"] - b["grad"]).max() <= 1e-13 * max(1.0, np.abs(a["grad"]).max()), c.name
        if not c.powered:                                                            # neuralNDCG.py:125 keeps the powered idcg
            plain = R._core(s, y, p._replace(transposed=False), tol)
            if (plain["idcg"] != 0).any():
                assert (a["idcg"][plain["idcg"] != 0] != plain["idcg"][plain["idcg"] != 0]).any(), c.name


def test_defects_the_max_norm_bar_lets_through():
    """for every defect model and every case it changes: does the entrywise contract catch it, does grad_close(rtol = 5e-4)?"""
    through = {}
    for wrong in R.WRONG:
        for c in R.CASES:
            if c.L > 129:
                continue
            ref, good, got = R.reference(c), R.transcription(c), R.transcription(c, wrong)
            if all(np.array_equal(good[k], got[k]) for k in OUTPUTS) and good["T"] == got["T"]:
                continue
            caught = max(_ratios(got, ref).values()) > 1.0 or not R.exact_ok(got, ref)
            if grad_close(got["grad"], ref["grad"], rtol=5e-4) and abs(float(got["loss"]) - ref["loss"]) <= 1e-5:
                through.setdefault(wrong, []).append((c.name, caught))
    for wrong, rows in sorted(through.items()):
        print("%s passes grad_close(5e-4) and a 1e-5 loss bar on: %s" % (wrong, "; ".join("%s (%s by the contract)" % (n, "outside a bar" if ok else "inside every bar: equivalent within rounding there") for n, ok in rows)))
        assert all(ok for n, ok in rows if n == R.NAMED[wrong]), wrong


def test_perturb_and_fold_references():
    rng = np.random.default_rng(3)
    s = rng.standard_normal((3, 8)).astype(R.F)
    y = rng.integers(0, 5, (3, 8)).astype(R.F)
    y[1, 5:] = R.PAD
    g = rng.standard_normal((2, 3, 8)).astype(R.F)
    out = R.perturb_ref(s, y, np.ones(3), 3.0, g, 0.1, True, False)
    assert out["s_pert"].shape == (6, 8) and out["k_rows"].tolist() == [8, 5, 8] * 2 and out["cnt_ps"] == 6.0
    sp32 = (np.log((s + abs(s.min())) + R.F(1e-10)).astype(R.F)[None] + (R.F(0.1) * g).astype(R.F)).astype(R.F).reshape(6, 8)
    assert not R.over(sp32, out["s_pert"], out["bar_s_pert"]).any()
    gp = rng.standard_normal((2, 24))
    for log_scores in (0, 1):
        ref, bar = R.fold_ref(gp.astype(R.F), s, log_scores)
        wt = (R.F(1) / ((s.ravel() + abs(s.min())) + R.F(1e-10))).astype(R.F) if log_scores else np.ones(24, R.F)
        gs = ((gp.astype(R.F)[0] + gp.astype(R.F)[1]).astype(R.F) * wt).astype(R.F)
        got = gs.copy()
        got[s.ravel() == s.min()] += R.F(np.sign(s.min()) * gs.sum(dtype=R.F))
        assert not R.over(got, ref, bar).any()
