"""tests/layernorm_ref.py on the CPU (no GPU), for every row of its case table: (a) the fp32 transcription of the kernels' arithmetic, in
the kernels' operation order, is inside every bar, so the bars are attainable; (b) every defect model puts at least one entry
outside its bar wherever it applies, so the bars discriminate; (c) the references are the oracle's custom_ln_fwd / custom_ln_bwd;
(d) the restated launch shapes and arm predicate are the source's; (e) the table launches every kernel instantiation and holds every
width and launch shape that the bit-for-bit tests (test_gpu_norm_head.py, test_gpu_tn_group_ln.py) rest on."""
import numpy as np
import pytest

from oracle import model_oracle as MO
from tests import layernorm_ref as R

HEAD = 64
ROW_LOCAL = ("no_gm", "D_for_Dm1", "tc_sign", "no_dres")          # of the backward: they change dx alone (every forward defect is row-local)


def _scale(c, opt):
    return R.keep_scale(opt.p, R.SEED, opt.word, c.rows, c.D) if opt.res else None


def _fwd_checks(c, X, opt, scale, got):
    """{output: (got, ref, bar)} of one forward, the statistics referred to the xsum it wrote"""
    v, mean, r, y = got
    res = X["res"] if opt.res else None
    xsum = (v, R.xsum_ref(X["x"], res, scale), R.xsum_bar(X["x"], res, scale))
    if R.over(*xsum).any():                                    # checked first, on its own: the rest is referred to a right xsum
        return dict(xsum=xsum)
    m64, r64, y64 = R.fwd_ref(v, X["a"], X["b"], c.eps)
    bm, br, by = R.fwd_bar(v, X["a"], X["b"], c.eps, R.is_vec(c))
    return dict(xsum=xsum, mean=(mean, m64, bm), rstd=(r, r64, br), y=(y, y64, by))


def _bwd_checks(c, opt, got, ref, bar):
    dx, part = got
    out = dict(dx=(dx, ref["dx"], bar["dx"]), partial=(part, ref["partial"], bar["partial"]))
    for reducer, tag in (("kernel", ""), ("group", "_group")):
        da, db = R.reduce_f32(part, reducer)
        out["da" + tag], out["db" + tag] = (da, ref["da"], bar["da" + tag]), (db, ref["db"], bar["db" + tag])
    return out


def _caught(checks):
    return any(R.over(*t).any() for t in checks.values())


@pytest.mark.parametrize("c", [pytest.param(c, id=c.name) for c in R.CASES])
def test_transcription_inside_every_bar_and_every_defect_outside(c):
    X = R.inputs(c)
    vec = R.is_vec(c)
    worst = {}
    # a defect of one row's arithmetic shows in that row: on the large cases those are run on the first HEAD rows (the special rows among
    # them), against the same references and bars; the transcription itself and the defects of the row walk take all rows
    head = slice(0, HEAD if c.rows * c.D >= R.LARGE else c.rows)
    cut = lambda v: None if v is None else v[head]          # noqa: E731
    Xh = dict(X, x=X["x"][head], res=X["res"][head])
    for opt in R.fwd_options(c):
        scale = _scale(c, opt)
        res = X["res"] if opt.res else None
        for k, t in _fwd_checks(c, X, opt, scale, R.fwd_f32(X["x"], res, scale, X["a"], X["b"], c.eps, vec)).items():
            worst["fwd " + k] = max(worst.get("fwd " + k, 0.0), R.worst(*t))
        for wrong in R.FWD_WRONG:
            why = R.fwd_applies(c, opt, wrong)
            if why is None:
                bad = R.fwd_f32(Xh["x"], cut(res), cut(scale), X["a"], X["b"], c.eps, vec, wrong=wrong)
                assert _caught(_fwd_checks(c, Xh, opt, cut(scale), bad)), "%s, %s: the forward defect %r is inside every bar" % (c.name, opt.name, wrong)
    _, mean, rstd, _ = R.fwd_f32(X["x"], None, None, X["a"], X["b"], c.eps, vec)
    shape = R.ln_bwd_shape(c.rows, c.D, vec)
    for opt in R.bwd_options(c):
        dres = X["dres"] if opt.dres else None
        args = (X["dy"], X["x"], X["a"], mean, rstd, dres, c.eps)
        ref, bar = R.bwd_ref(*args, shape=shape), R.bwd_bar(*args, vec, shape)
        for k, t in _bwd_checks(c, opt, R.bwd_f32(*args, vec, shape), ref, bar).items():
            worst["bwd " + k] = max(worst.get("bwd " + k, 0.0), R.worst(*t))
        shift = R.tc_shift(X["dy"], X["x"], X["a"], mean, rstd, c.eps)
        for wrong in R.BWD_WRONG:
            why = R.bwd_applies(c, opt, wrong, shift, bar["dx"])
            if why is not None and wrong == "D_for_Dm1":
                assert c.rows == 1 and c.D >= 1024, "%s: %s" % (c.name, why)          # chance, and only where one wide row is all there is
                print("%s, %s: %s cannot show: %s" % (c.name, opt.name, wrong, why))
            if why is None and wrong in ROW_LOCAL:
                bad = R.bwd_f32(*[cut(v) if isinstance(v, np.ndarray) and v.shape[0] == c.rows else v for v in args], vec, (1, 4), wrong=wrong)[0]
                assert R.over(bad, ref["dx"][head], bar["dx"][head]).any(), "%s, %s: the backward defect %r is inside the bar of dx" % (c.name, opt.name, wrong)
            elif why is None:
                bad = _bwd_checks(c, opt, R.bwd_f32(*args, vec, shape, wrong=wrong), ref, bar)
                assert _caught(bad), "%s, %s: the backward defect %r is inside every bar" % (c.name, opt.name, wrong)
                if wrong == "second_trip_shifted":            # the sums are right: only the partial rows can tell
                    assert R.over(*bad["partial"]).any()
    print("%s [%s]: worst error / bar  %s" % (c.name, ", ".join(sorted(R.kernels(c))), "  ".join("%s %.3g" % kv for kv in sorted(worst.items()))))
    assert max(worst.values()) <= 1.0, worst


def test_every_defect_applies_somewhere_on_every_arm():
    for vec in (False, True):
        cs = [c for c in R.CASES if R.is_vec(c) == vec]
        for wrong in R.FWD_WRONG:
            if vec and wrong in ("mean_padded", "sq_tail_dropped"):
                continue                                       # the register layout has no partial trip: D % 256 == 0
            assert any(R.fwd_applies(c, o, wrong) is None for c in cs for o in R.fwd_options(c)), (vec, wrong)
        for wrong in R.BWD_WRONG:
            assert any(R.bwd_applies(c, o, wrong) is None for c in cs for o in R.bwd_options(c)), (vec, wrong)


@pytest.mark.parametrize("rows,D,eps", [(37, 20, 1e-6), (37, 256, 1e-3), (3, 2, 1e-6)])
def test_references_are_the_oracles(rows, D, eps):
    """custom_ln_fwd, then custom_ln_bwd on its own cache, in fp64 == the module's references handed the forward's statistics"""
    c = R.Case("oracle", rows, D, eps, None, True)
    X = R.inputs(c)
    x, a, b, dy = (R.f64(X[k]) for k in ("x", "a", "b", "dy"))
    y, cache = MO.custom_ln_fwd(x, a, b, R.w(eps))
    grads = {}
    dx = MO.custom_ln_bwd(cache, a, dy, grads, "n")
    mean, rstd, y_ref = R.fwd_ref(X["x"], X["a"], X["b"], eps)
    assert np.array_equal(y, y_ref) and np.array_equal(rstd, cache[2][:, 0]) and np.array_equal(mean, x.mean(-1))
    shape = R.ln_bwd_shape(rows, D, False)
    got = R.bwd_ref(X["dy"], X["x"], X["a"], mean, rstd, X["dres"], eps, shape=shape)
    live = cache[1][:, 0] > 0                                  # 1 / r - eps loses the constant row's std = 0 to fp64 rounding: tc is 0 either way
    assert live.sum() >= rows - 1
    for name, u, v in (("dx", got["dx"] - R.f64(X["dres"]), dx), ("da", got["da"], grads["n.a_2"]), ("db", got["db"], grads["n.b_2"])):
        # 1 / r - eps in fp64 carries 2^-53 (std + eps) / std relative into tc: 1e-9 is far above that and far below u
        assert np.abs(u - v).max() <= 1e-9 * np.abs(v).max(), name
    assert np.allclose(got["partial"].sum(0), np.stack([got["da"], got["db"]]), rtol=1e-12, atol=1e-12 * np.abs(dy).sum(0).max())
    assert got["partial"].shape == (shape[0], 2, D)


def test_restated_launch_shapes_are_the_sources():
    k = R.source_constants()
    assert (k["g16"], k["wide_rows"], k["bwd_cap"], k["max_bwd_d"]) == (R.LN_BWD_G16, R.WIDE_ROWS, R.BWD_GRID_CAP, R.MAX_BWD_D)
    assert k["fwd_cap"] == k["fwd_vec_cap"] == R.FWD_GRID_CAP
    assert (k["vec_mod"], k["vec_max_d"], k["vec_align"], k["wide_max_d"]) == (256, 1024, 16, 512)
    assert R.ln_vec_ok(512, (0, 4096, 16)) and not R.ln_vec_ok(512, (4096, 4100)) and not R.ln_vec_ok(1280) and not R.ln_vec_ok(136)
    assert R.ln_bwd_shape(R.WIDE_ROWS, 512, True) == (R.LN_BWD_G16, 16) and R.ln_bwd_shape(R.WIDE_ROWS - 1, 512, True) == (320, 4)
    assert R.ln_bwd_shape(R.WIDE_ROWS, 768, True) == (320, 4) and R.ln_bwd_shape(R.WIDE_ROWS, 512, False) == (320, 4)
    assert R.ln_bwd_shape(1, 2, False) == (1, 4) and R.ln_bwd_shape(37, 256, True) == (3, 4) and R.ln_bwd_shape(5127, 136, False) == (320, 4)
    assert R.fwd_grid(5127, False) == 1024 and R.fwd_grid(37, False) == 10 and R.fwd_grid(37, True) == 5 and R.fwd_grid(R.WIDE_ROWS + 5, True) == 1024
    assert R.workspace_bytes(37, 256) == 320 * 2 * 256 * 4 and R.workspace_bytes(0, 256) == 0


def test_the_table_reaches_every_instantiation_and_every_shape_of_the_bit_for_bit_tests():
    launched = set().union(*[R.kernels(c) for c in R.CASES])
    assert launched == set(R.ALL_KERNELS), sorted(set(R.ALL_KERNELS) ^ launched)
    table = {(c.rows, c.D) for c in R.CASES if R.is_vec(c)}
    # the grid-stride loops take a second trip: scalar forward (1024 x 4 rows) and backward (320 x 16), vec forward (1024 x 8), vec backward
    assert any(not R.is_vec(c) and c.rows > 4096 for c in R.CASES) and any(R.is_vec(c) and c.rows > 2 * 8192 for c in R.CASES)
    assert any(R.is_vec(c) and c.D > 512 and c.rows > 320 * 16 for c in R.CASES)
    assert {c.misaligned for c in R.CASES if c.D == 512} == {None, "in", "out"}
    same = [R.inputs(c) for c in R.CASES if (c.rows, c.D, c.eps) == (37, 512, 1e-6)]          # both arms on the same rows
    assert len(same) == 3 and all(np.array_equal(same[0][k], X[k]) for X in same[1:] for k in same[0])
    from tests import test_gpu_norm_head as NH
    from tests import test_gpu_tn_group_ln as TG
    assert NH.WIDE_ROWS == TG.WIDE_ROWS == R.WIDE_ROWS
    assert set(NH.CASES) <= table, sorted(set(NH.CASES) - table)
    assert {(rows, D) for _, _, rows, D in TG.SHAPES} <= table
    shapes = {R.ln_bwd_shape(c.rows, c.D, True) for c in R.CASES if R.is_vec(c)}
    assert {R.ln_bwd_shape(rows, D, True) for _, _, rows, D in TG.SHAPES} <= shapes
