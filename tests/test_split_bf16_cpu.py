"""The split-bf16 arithmetic of allrank_amd/csrc/ltrx_gemm.hip on the CPU (tests/gemm_ref.py): what the split itself costs,
as a BOUND, entry by entry, on operands that are not normalised.

bf16 keeps 8 significand bits; rounding to nearest gives |x - bf16(x)| <= u |x| with unit round-off u = 2^-8 (not 2^-9: 2^-9 is
the TYPICAL error of a random mantissa).  With hi = bf16(x), lo = bf16(x - hi), lo2 = bf16(x - hi - lo) (the fp32 subtractions
are exact) and e_n = x - (the first n terms):
    |e_1| <= u |x|,  |e_2| <= u^2 |x|,  |e_3| <= u^3 |x|,      |hi| <= (1 + u) |x|,  |lo| <= u (1 + u) |x|,  |lo2| <= u^2 (1 + u) |x|.
Per product a b, the error of what the kernels sum instead:
  precision 2 (hi hi):                    a b - ah bh = a e_1(b) + e_1(a) bh                  <= u (2 + u) |a b|  <=  2 u (1 + u)
  precision 0 (hi hi + hi lo + lo hi):    a e_2(b) + e_2(a) b - e_2(a) e_2(b) + al bl
                                          <= (2 u^2 + u^4 + u^2 (1 + u)^2) |a b|                    <=  3 u^2 (1 + 2 u)
  precision 1 (+ lo lo + hi lo2 + lo2 hi): a e_3(b) + e_3(a) b - e_3 e_3 + al bl2 + al2 bl + al2 bl2
                                          <= (2 u^3 + u^6 + (2 u^3 + u^4) (1 + u)^2) |a b|          <=  4 u^3 (1 + 2 u)
i.e. 7.84e-3, 4.61e-5 and 2.40e-7 of sum_k |a||b|, entrywise.  The figures the sources used to quote (2^-9, 3 * 2^-18, 2^-26)
are typical values: the tests below show each of them exceeded."""
import numpy as np
import pytest

from tests import gemm_ref as R

# what include/ltrx.h and ltrx_gemm.hip quoted before as if they were bounds
TYPICAL = {2: 2.0 ** -9, 0: 3 * 2.0 ** -18, 1: 2.0 ** -26}


def test_split_terms_follow_split4_and_the_unit_roundoff_is_2_to_the_minus_8():
    """hi / lo / lo2 per element: residuals bounded by u, u^2, u^3 with u = 2^-8, and NOT by the halved constants."""
    rng = np.random.default_rng(0)
    x = (1.0 + rng.random(1 << 16)).astype(np.float32) * (2.0 ** rng.integers(-40, 41, 1 << 16)).astype(np.float32)
    hi, lo, lo2 = R.split(x, 3)
    assert R.split(x, 2)[2] is None and np.array_equal(R.split(x, 2)[1], lo) and np.array_equal(R.split(x, 1)[0], hi)
    x64 = x.astype(np.float64)
    e1 = float((np.abs(x64 - hi) / np.abs(x64)).max())
    e2 = float((np.abs(x64 - hi - lo) / np.abs(x64)).max())
    e3 = float((np.abs(x64 - hi - lo - lo2) / np.abs(x64)).max())
    assert 2.0 ** -9 < e1 <= 2.0 ** -8, "max |x - hi| / |x| = %.4g" % e1
    assert 2.0 ** -18 < e2 <= 2.0 ** -16, "max |x - hi - lo| / |x| = %.4g (the sources said 2^-18 = %.4g)" % (e2, 2.0 ** -18)
    assert e3 <= 2.0 ** -24, "max |x - hi - lo - lo2| / |x| = %.4g" % e3
    # every term is a bf16 value: its low 16 bits are zero
    for t in (hi, lo, lo2):
        assert not (t.view(np.uint32) & 0xFFFF).any()
    z = np.array([0.0, -0.0, np.inf, -np.inf, np.nan], np.float32)
    zh, zl, _ = R.split(z, 3)
    assert np.array_equal(zh[:2], z[:2]) and np.all(zl[:2] == 0) and np.isinf(zh[2:4]).all() and np.isnan(zl[2:]).all()


@pytest.mark.parametrize("prec", [2, 0, 1])
def test_emulated_products_stay_within_the_worst_case_split_bound_entrywise(prec):
    """emulate_nt / emulate_tn against the exact fp64 product, every entry against ITS OWN sum_k |a||b|, rows of A and B scaled by
    2^[-40, 40] and columns of A by 2^[-6, 6]; the bound is SPLIT_BOUND (derivation above), and the previously documented figure is
    shown to be exceeded (for the precisions whose worst case a random draw comes near)."""
    worst, where = 0.0, None
    for (M, N, K, seed) in [(65, 130, 32, 1), (129, 127, 36, 2), (64, 257, 96, 3), (33, 40, 2048, 4), (300, 64, 32, 5)]:
        rng = np.random.default_rng(seed)
        A, B = R.scaled_operands(rng, M, N, K)
        exact = A.astype(np.float64) @ B.astype(np.float64).T
        S = R.abs_nt(A, B)
        for kind in ("nt", "tn"):
            if kind == "nt":
                em = R.emulate_nt(A, B, prec)
            else:
                em = R.emulate_tn(np.ascontiguousarray(A.T), np.ascontiguousarray(B.T), prec)      # contraction over the rows
            assert em.shape == exact.shape
            with np.errstate(invalid="ignore", divide="ignore"):
                ratio = np.where(S > 0, np.abs(em - exact) / S, 0.0)
            assert np.all(em[S == 0] == 0)                                                        # the all-zero rows
            m = float(ratio.max())
            if m > worst:
                worst, where = m, (kind, M, N, K) + tuple(int(v) for v in np.unravel_index(int(ratio.argmax()), ratio.shape))
            assert m <= R.SPLIT_BOUND[prec], "precision %d %s %s: worst entrywise error %.4g of S above the bound %.4g" % (
                prec, kind, (M, N, K), m, R.SPLIT_BOUND[prec])
    msg = "precision %d: measured worst entrywise error %.4g of S at %s; bound %.4g; previously documented %.4g" % (
        prec, worst, where, R.SPLIT_BOUND[prec], TYPICAL[prec])
    print(msg)
    assert worst <= R.SPLIT_BOUND[prec], msg
    assert worst > TYPICAL[prec], msg          # the documented figure was a typical value, not a bound


def test_next_cheaper_precision_is_outside_the_accumulation_bar():
    """the bar the GPU contract uses ((P K + 3) 2^-24 of S, no measured number in it) separates the precision codes: the
    one-product sum fails the three-product bar at every K <= 160 ((3 K + 3) 2^-24 <= 2.9e-5 against a dropped hi lo term of up to
    2^-8); the three-product sum fails the six-product bar at the small K of the contract's cases (the dropped lo lo term is at most
    2^-16 (1 + u)^2 = 1.5e-5 of |a b|, (6 K + 3) 2^-24 is below that up to K = 41 -- at K = 160 a missing lo lo product hides inside
    the accumulation bound, which is why the six-product cases keep K small)."""
    rng = np.random.default_rng(7)
    for (K, pairs) in ((4, ((0, 2), (1, 0))), (20, ((0, 2), (1, 0))), (160, ((0, 2),))):
        A, B = R.scaled_operands(rng, 65, 130, K)
        S = R.abs_nt(A, B)
        for (prec, cheaper) in pairs:
            bar = R.bar_nt(S, K, prec)
            good, bad = R.emulate_nt(A, B, prec), R.emulate_nt(A, B, cheaper)
            frac = float((np.abs(bad - good) > bar).mean())
            assert frac > 0.0, (K, prec, cheaper)


def test_epilogue64_forms():
    rng = np.random.default_rng(3)
    acc = rng.standard_normal((5, 8))
    bias, aux = rng.standard_normal(8), rng.standard_normal((5, 8))
    from oracle import dropout_oracle as D
    ks = D.keep_scale(0.25, 9, 2, (5, 8)).astype(np.float64)
    assert 0 < (ks == 0).sum() < 40
    out, pre = R.epilogue64(acc, 0, bias)
    assert np.array_equal(out, acc + bias) and np.array_equal(pre, out)
    assert np.array_equal(R.epilogue64(acc, 1, bias, None, 0.25, 9, 2)[0], np.maximum(acc + bias, 0) * ks)
    assert np.array_equal(R.epilogue64(acc, 2, None, aux, 0.25, 9, 2)[0], np.where(aux > 0, acc * float(np.float32(1) / np.float32(0.75)), 0))
    assert np.array_equal(R.epilogue64(acc, 3, bias, aux, 0.25, 9, 2)[0], (acc + bias) * ks + aux)
    assert np.array_equal(R.epilogue64(acc, 3, bias, aux)[0], acc + bias + aux)
