"""tests/fcstep_ref.py holds what it promises, without a GPU: on every case of the table the fp32 transcription of the kernel is inside
every stage's bar (so the bars are not too tight for a correct kernel), every defect model is outside a bar on every case it names (so
they bite), the share of ReLU pre-activations whose sign the reference cannot decide stays within its cap, the split bound holds, and
the table reaches every instantiation and every branch of the host's dispatch.  tests/test_gpu_fcstep_contract.py runs the same
comparison code on the device's outputs."""
import numpy as np
import pytest

from tests import fcstep_ref as R

CUS = R.CPU_CUS
UNDECIDABLE_CAP = 1e-3
_MEMO = {}


def _case(c):
    if c.name not in _MEMO:
        _MEMO.clear()                                   # (one case's arrays at a time)
        cr = R.resolve(c, CUS)
        X = R.inputs(cr, CUS)
        _MEMO[c.name] = (cr, X, R.transcribe(cr, X, CUS))
    return _MEMO[c.name]


IDS = [pytest.param(c, id=c.name) for c in R.CASES]


def test_constants_match_the_source():
    k = R.source_constants()
    assert (k["rows"], k["maxf"], k["maxh"], k["nld"]) == (R.FC_ROWS, R.FC_MAXF, R.FC_MAXH, R.FC_NLD)
    assert (k["ksmall"], k["kmax"], k["pstride"], k["ws_cap"]) == (R.FL_KSMALL, R.FL_KMAX, R.FL_PSTRIDE, R.WS_WG_CAP)


@pytest.mark.parametrize("c", IDS)
def test_transcription_is_inside_every_bar(c):
    cr, X, got = _case(c)
    rat = R.ratios(cr, X, got, CUS)
    print("%s: %s" % (c.name, ", ".join("%s %.3g" % kv for kv in rat.items())))
    assert all(v <= 1.0 for v in rat.values()), rat
    # the optional outputs are outputs only
    assert set(rat) >= {"scores", "dscores", "loss", "dW1", "db1", "dw_out", "db_out", "grads padding"}


@pytest.mark.parametrize("c", IDS)
def test_every_defect_is_outside_a_bar_where_it_applies(c):
    cr, X, _ = _case(c)
    for wrong in R.wrongs(c):
        why = R.applies(cr, X, CUS, wrong)
        rat = R.ratios(cr, X, R.transcribe(cr, X, CUS, wrong), CUS)
        top = max(rat.values())
        print("%s, %s: %s" % (c.name, wrong, "worst error / bar %.3g" % top if why is None else "not applicable: " + why))
        if why is None:
            assert top > 1.0, (c.name, wrong, rat)


@pytest.mark.parametrize("c", IDS)
def test_relu_pattern_is_decidable_and_the_split_bound_holds(c):
    cr, X, _ = _case(c)
    if c.kind != "fc":
        return
    hid, pre, bar, scale, true = R.hidden_ref(X["x"], X["params"], c.H, c.act)
    share = float(R.relu_undecidable(pre, bar).mean())
    print("%s: %.3g of the pre-activations are within the bar of 0" % (c.name, share))
    assert share <= UNDECIDABLE_CAP
    assert (np.abs(pre - true) <= R.SPLIT_BOUND[0] * scale).all()
    # ... and for the weight gradient's products, with the transcription's dh
    got = _case(c)[2]
    dh = R.dh_exact(got["dscores"], got["hidden"], X["params"], c.F, c.H, c.act)
    n = dh.shape[0] * dh.shape[1]
    x2, d2 = X["x"].reshape(n, c.F), dh.reshape(n, c.H)
    xh, xl = R._split64(x2)
    dhh, dhl = R._split64(d2)
    em = dhh.T @ xl + dhl.T @ xh + dhh.T @ xh
    assert (np.abs(em - R.f64(d2).T @ R.f64(x2)) <= R.SPLIT_BOUND[0] * (np.abs(R.f64(d2)).T @ np.abs(R.f64(x2)))).all()


def test_every_defect_applies_somewhere():
    hit = {}
    for c in R.CASES:
        cr, X, _ = _case(c)
        for wrong in R.wrongs(c):
            if R.applies(cr, X, CUS, wrong) is None:
                hit.setdefault((c.kind, wrong), []).append(c.name)
    for kind, ws in (("fc", R.FC_WRONG), ("lin", R.LIN_WRONG)):
        for wrong in ws:
            if wrong == "no_D_b1":                      # the one defect no input can show: see fcstep_ref.applies
                assert (kind, wrong) not in hit
                continue
            assert len(hit.get((kind, wrong), [])) >= 2, (kind, wrong)


def test_table_reaches_every_instantiation_and_branch():
    fc = [c for c in R.CASES if c.kind == "fc"]
    lin = [c for c in R.CASES if c.kind == "lin"]
    assert {R.kernel_name(c) for c in R.CASES} == set(R.ALL_KERNELS)
    assert {c.F for c in fc} >= {4, 12, 36, 44, 128, 132, 136, 144}
    assert {c.H for c in fc} >= {1, 16, 17, 33, 80, 96}
    assert {R.nhb_of(c.H) for c in fc} >= {2, 3, 5, 6}
    assert {c.L for c in fc} >= {1, 16, 17, 32, 33, 127, 128, 129, 240, 256}
    assert all(R.supported(c.L, c.F, c.H) for c in R.CASES)
    # the plain staging loop beyond FC_NLD * blockDim float4s, at both block sizes
    loop = {(c.L, c.F, c.H) for c in fc if c.L * (c.F // 4) > R.FC_NLD * 128 * R.nhb_of(c.H)}
    assert {(256, 144, 16), (240, 136, 33)} <= loop
    # B: the reduce's group boundary, one / two / three slates per workgroup
    assert {c.B for c in fc} >= {1, 63, 64, 65, (1, 0), (1, 1), (2, 1)}
    for c in fc:
        if not isinstance(c.B, int):
            assert c.L * c.F * c.H <= 33 * 36 * 20 * 2
    # the linear kernel at its switch: 11 passes, 12 passes, 13 passes; 1, 2, 3, 4 slates per workgroup (register double-buffering)
    assert {(c.L, c.F): R.lin_shape(c.L, c.F)[1:] for c in lin if c.L >= 240} == {(240, 136): (11, 11), (243, 136): (12, 13), (256, 144): (13, 13)}
    assert {c.B for c in lin} >= {(1, 0), (1, 1), (2, 1), (3, 1)}
    for kind in ("fc", "lin"):
        cs = [c for c in R.CASES if c.kind == kind]
        assert {c.adam for c in cs} == {None, "l2", "adamw"} and {c.t0 for c in cs if c.adam} == {0, 9}
        assert {c.weights for c in cs} == {"init", "big"} and any(c.div_mul != 1.0 for c in cs)
        seen, under, top = set(), 0, 0.0
        for c in cs:
            cr, X, got = _case(c)
            valid = X["y"] != R.PAD
            seen |= {R.pattern(c, b) for b in range(min(X["B"], len(R.PATTERNS)))}
            under += int(X["underflow"])
            if X["underflow"]:
                ln = R.listnet_ref(got["scores"], X["y"], cr.eps, cr.div)
                assert ((ln["P"] < R.FLT_MIN) & valid).any(), c.name
            if c.weights == "big":
                top = max(top, float(np.abs(got["scores"][valid]).max()))
            assert (c.H % 4 != 0) == (R.layout(c.F, c.H)[4] != c.H * c.F + 2 * c.H + 4)
        assert seen == set(R.PATTERNS) and under >= 3 and top >= 29.0, (kind, seen, under, top)
    assert any(c.H % 4 for c in fc) and any(c.H % 4 for c in lin)
    # the workspace the entry points promise covers what the kernels write, on any device up to 1024 compute units
    for c in R.CASES:
        for cus in (64, 256, 304, 1024):
            B = R.batch(c, cus)
            assert R.ws_used(c.kind, B, c.F, c.H, cus) <= R.ws_bytes(c.kind, B, c.F, c.H)
