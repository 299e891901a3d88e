"""-m gpu: the encoder's final norm fused with the d_output == 1 score head (ltrx_norm_head_fwd, ltrx_norm_head_bwd_partial,
ltrx_norm_head_wgrad).

Kernel level, per (rows, D): everything the two-kernel composition produces -- mean, rstd, LN(x), the scores, dx, d a_2, d b_2 and the
head's own dw, db -- is compared BIT FOR BIT with ltrx_layernorm_fwd -> ltrx_score_head_fwd -> ltrx_score_head_bwd ->
ltrx_layernorm_bwd_partial -> ltrx_reduce_group on the same inputs.  (A training run doubles a rounding-sized difference in the head's
gradients about every step -- ApproxNDCG's d loss / d bias is pure rounding noise that Adam turns into a full-size update -- so the
head's gradients are recomputed in ltrx_score_head_bwd's own order rather than merely held to a bar.)  The scores and the head's
gradients are also held to fp64 with a-priori bars: the computed value of a sum of products whose longest chain of roundings is k
long differs from the exact one by at most gam(k) * sum |terms| (gam(k) = k u / (1 - k u), u = 2^-24).
  scores:   k = D / 64 (a lane's fma chain) + 6 (wave tree) + 1 (bias);  terms y[r, c] w[c] and bias, y = the fp32 LN(x)
  dw_head:  k = rows a wave walks + 4 (waves of a workgroup) + partial rows / 16 + 1 + 16 (ltrx_score_head_reduce_kernel) + 2 (the
            recomputed y rounds as the stored one did; one more covers the product);  terms ds[r] y[r, c]
  db_head:  the same k;  terms ds[r]
Shapes: 37 rows (a few rows per wave, ragged), LTRX_LN_BWD_WIDE_ROWS + 5 (the 16-wave backward arm the flagship step takes, ragged
tail) and LTRX_LN_BWD_WIDE_ROWS - 1 (the 4-wave arm just below the switch); one constant row (std = 0: the stdv > 0 guard), one row
with ds = 0, one zero in a_2.

Engine level: one FusedTrainer step at 4 x 16, d_model 256, with the fused pair on and forced off (padded, compact on ragged
lengths, dropout 0.1): loss, scores, scorer output, every gradient and every parameter bit-equal."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
EPS = 1e-6
EINVAL, EUNSUPPORTED = -1, -2


def _wide_rows():
    """LTRX_LN_BWD_WIDE_ROWS as csrc/ltrx_layernorm.hip defines it (16 * 4 * LTRX_LN_BWD_G16), read from the source"""
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "allrank_amd", "csrc", "ltrx_layernorm.hip")).read()
    g16 = int(re.search(r"#define LTRX_LN_BWD_G16 (\d+)", src).group(1))
    assert re.search(r"#define LTRX_LN_BWD_WIDE_ROWS \(16 \* 4 \* LTRX_LN_BWD_G16\)", src)
    return 16 * 4 * g16


WIDE_ROWS = _wide_rows()
GUARD = 64                                # floats of sentinel behind every output


def gam(k):
    return k * U / (1.0 - k * U)


def _libs():
    from allrank_amd import _lib as LB
    return LB, LB.lib()


def _out(*shape):
    """an output of the given shape at the head of a NaN-filled buffer with GUARD floats behind it; (view, check the guard)"""
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    return buf[:n].view(*shape), lambda: bool(torch.isnan(buf[n:]).all())


def _inputs(rows, D):
    rng = np.random.default_rng(1000 * D + rows)
    x = (3.0 * rng.standard_normal((rows, D))).astype(np.float32)
    x[5] = 1.25                                                   # std = 0
    ds = rng.standard_normal(rows).astype(np.float32)
    ds[7] = 0.0
    a, b, w = (rng.standard_normal(D).astype(np.float32) for _ in range(3))
    a[3] = 0.0
    bias = rng.standard_normal(1).astype(np.float32)
    return tuple(torch.tensor(v, device=DEV) for v in (x, ds, a, b, w, bias))


def _reduce(lib, LB, entries):
    n = len(entries)
    vp = ctypes.c_void_p * n
    LB.check(lib.ltrx_reduce_group(n, vp(*[e[0] for e in entries]), (ctypes.c_int * n)(*[e[1] for e in entries]),
                                   (ctypes.c_size_t * n)(*[e[2] for e in entries]), (ctypes.c_size_t * n)(*[e[3] for e in entries]),
                                   vp(*[e[4].data_ptr() for e in entries]), None), "reduce_group")


def _two_kernel(rows, D, x, ds, a, b, w, bias):
    """the composition the step ran before: LayerNorm forward, head forward, head backward, LayerNorm backward + reduce"""
    LB, lib = _libs()
    P = LB.ptr
    y, mean, rstd, sc = torch.empty_like(x), torch.empty(rows, device=DEV), torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
    LB.check(lib.ltrx_layernorm_fwd(P(x), None, P(a), P(b), rows, D, EPS, None, P(y), P(mean), P(rstd), 0.0, 0, None, None), "ln_fwd")
    LB.check(lib.ltrx_score_head_fwd(P(y), P(w), P(bias), rows, D, P(sc), None), "head_fwd")
    dxf, dw, db = torch.empty_like(x), torch.empty_like(w), torch.empty_like(bias)
    ws_h = torch.empty(max(lib.ltrx_score_head_bwd_workspace_bytes(rows, D), 64), dtype=torch.uint8, device=DEV)
    LB.check(lib.ltrx_score_head_bwd(P(ds), P(y), P(w), rows, D, P(dxf), P(dw), P(db), P(ws_h), None), "head_bwd")
    dx, da, dbn = torch.empty_like(x), torch.empty_like(a), torch.empty_like(b)
    ws = torch.empty(max(lib.ltrx_layernorm_bwd_workspace_bytes(rows, D), 64), dtype=torch.uint8, device=DEV)
    pr = ctypes.c_int(0)
    LB.check(lib.ltrx_layernorm_bwd_partial(P(dxf), P(x), P(a), P(mean), P(rstd), None, rows, D, EPS, P(dx), P(ws), ctypes.byref(pr),
                                            None), "ln_bwd_partial")
    _reduce(lib, LB, [(ws.data_ptr(), pr.value, 2 * D, D, da), (ws.data_ptr() + 4 * D, pr.value, 2 * D, D, dbn)])
    head_rows = lib.ltrx_score_head_bwd_workspace_bytes(rows, D) // (4 * (D + 1))          # its workgroups, one partial row each
    return dict(y=y, mean=mean, rstd=rstd, scores=sc, dx=dx, da=da, db=dbn, dw_head=dw, db_head=db, partial_rows=pr.value,
                head_rows=head_rows)


CASES = [(37, 256), (37, 512), (37, 768), (37, 1024), (WIDE_ROWS + 5, 256), (WIDE_ROWS + 5, 512), (WIDE_ROWS + 5, 1024),
         (WIDE_ROWS - 1, 512)]


@pytest.mark.parametrize("rows,D", CASES)
def test_fused_pair_against_the_two_kernel_composition_and_fp64(rows, D):
    LB, lib = _libs()
    P = LB.ptr
    x, ds, a, b, w, bias = _inputs(rows, D)
    keep = [t.clone() for t in (x, ds, a, b, w, bias)]
    ref = _two_kernel(rows, D, x, ds, a, b, w, bias)

    # ---- forward, with and without the optional LN(x) output
    for want_y in (True, False):
        (sc, g0), (mean, g1), (rstd, g2), (y, g3) = _out(rows), _out(rows), _out(rows), _out(rows, D)
        LB.check(lib.ltrx_norm_head_fwd(P(x), P(a), P(b), P(w), P(bias), rows, D, EPS, P(sc), P(mean), P(rstd), P(y) if want_y else None,
                                        None), "norm_head_fwd")
        assert g0() and g1() and g2() and g3(), "wrote past an output"
        assert torch.equal(mean, ref["mean"]) and torch.equal(rstd, ref["rstd"])
        assert torch.equal(y, ref["y"]) if want_y else bool(torch.isnan(y).all())
        assert torch.equal(sc, ref["scores"]), "scores differ from ltrx_score_head_fwd on the stored LN(x)"
    assert float(rstd[5]) == float(np.float32(1.0) / np.float32(EPS)) and float(mean[5]) == 1.25
    y64, w64 = ref["y"].double(), w.double()
    s_ref = y64 @ w64 + bias.double()
    s_bar = gam(D // 64 + 7) * ((y64.abs() @ w64.abs()) + bias.double().abs())
    r = float(((sc.double() - s_ref).abs() / s_bar).max())
    print("scores %dx%d: worst error / bar %.4g" % (rows, D, r))
    assert r <= 1.0

    # ---- backward
    nbytes = lib.ltrx_norm_head_bwd_workspace_bytes(rows, D)
    assert nbytes == lib.ltrx_layernorm_bwd_workspace_bytes(rows, D)
    ws = torch.zeros(nbytes + 256, dtype=torch.uint8, device=DEV)
    ws[nbytes:] = 0xA5
    (dx, g0), (da, g1), (dbn, g2), (dwh, g3), (dbh, g4) = _out(rows, D), _out(D), _out(D), _out(D), _out(1)
    pr = ctypes.c_int(0)
    LB.check(lib.ltrx_norm_head_bwd_partial(P(ds), P(x), P(a), P(w), P(mean), P(rstd), rows, D, EPS, P(dx), P(ws), ctypes.byref(pr), None),
             "norm_head_bwd_partial")
    hbytes = lib.ltrx_score_head_bwd_workspace_bytes(rows, D)
    ws_h = torch.zeros(hbytes + 256, dtype=torch.uint8, device=DEV)
    ws_h[hbytes:] = 0xA5
    LB.check(lib.ltrx_norm_head_wgrad(P(ds), P(x), P(a), P(b), P(mean), P(rstd), rows, D, P(dwh), P(dbh), P(ws_h), None), "norm_head_wgrad")
    assert bool((ws_h[hbytes:] == 0xA5).all()), "wrote past the head workspace"
    assert pr.value == ref["partial_rows"] and 0 < pr.value * 2 * D * 4 <= nbytes      # the LayerNorm backward's own grid, either arm
    assert bool((ws[nbytes:] == 0xA5).all()), "wrote past the workspace"
    pw, base = 2 * D, ws.data_ptr()
    _reduce(lib, LB, [(base, pr.value, pw, D, da), (base + 4 * D, pr.value, pw, D, dbn)])
    assert g0() and g1() and g2() and g3() and g4(), "wrote past an output"
    assert torch.equal(dx, ref["dx"]), "dx differs from ltrx_score_head_bwd + ltrx_layernorm_bwd_partial"
    assert torch.equal(da, ref["da"]) and torch.equal(dbn, ref["db"])
    assert not dx[7].any()                                                    # ds = 0: no gradient into that row
    assert torch.equal(dwh, ref["dw_head"]) and torch.equal(dbh, ref["db_head"]), "the head's gradients differ from ltrx_score_head_bwd's"
    hg = ref["head_rows"]                                                     # ltrx_score_head_bwd's grid of 4-wave workgroups
    k = -(-rows // (hg * 4)) + 4 + -(-hg // 16) + 1 + 16 + 2
    ds64 = ds.double()
    dw_ref, dw_bar = ds64 @ y64, gam(k) * (ds64.abs() @ y64.abs())
    r = float(((dwh.double() - dw_ref).abs() / dw_bar).max())
    print("dw_head %dx%d: k = %d, worst error / bar %.4g" % (rows, D, k, r))
    assert r <= 1.0
    r = abs(float(dbh.double().item()) - float(ds64.sum())) / (gam(k) * float(ds64.abs().sum()))
    print("db_head %dx%d: worst error / bar %.4g" % (rows, D, r))
    assert r <= 1.0
    for t, t0 in zip((x, ds, a, b, w, bias), keep):
        assert torch.equal(t, t0), "an input was written"


def test_the_cases_straddle_the_switch_between_the_backward_s_two_arms():
    """the rows of CASES named after LTRX_LN_BWD_WIDE_ROWS do sit on either side of it: the library reports another partial-row count
    (another grid) just below than just above, at the width that has both arms, and the fused backward reports the same ones"""
    LB, lib = _libs()
    P = LB.ptr
    D, counts = 512, []
    for rows in (WIDE_ROWS - 1, WIDE_ROWS + 5):
        x, ds, a, b, w, bias = _inputs(rows, D)
        ref = _two_kernel(rows, D, x, ds, a, b, w, bias)
        ws = torch.zeros(lib.ltrx_norm_head_bwd_workspace_bytes(rows, D), dtype=torch.uint8, device=DEV)
        dx, pr = torch.empty_like(x), ctypes.c_int(0)
        LB.check(lib.ltrx_norm_head_bwd_partial(P(ds), P(x), P(a), P(w), P(ref["mean"]), P(ref["rstd"]), rows, D, EPS, P(dx), P(ws),
                                                ctypes.byref(pr), None), "norm_head_bwd_partial")
        assert pr.value == ref["partial_rows"]
        counts.append(pr.value)
    assert counts[0] != counts[1], counts


def test_unsupported_widths_and_alignment_are_refused_before_launching():
    LB, lib = _libs()
    P = LB.ptr
    buf = torch.zeros(64 * 1280 + 8, dtype=torch.float32, device=DEV)
    v = torch.zeros(1284, dtype=torch.float32, device=DEV)
    o = torch.full((64,), float("nan"), dtype=torch.float32, device=DEV)
    pr = ctypes.c_int(-7)
    ws = torch.zeros(lib.ltrx_norm_head_bwd_workspace_bytes(64, 1024), dtype=torch.uint8, device=DEV)

    def fwd(D, x=buf, a=v):
        return lib.ltrx_norm_head_fwd(P(x), P(a), P(v), P(v), P(v), 8, D, EPS, P(o), P(o), P(o), None, None)

    def bwd(D, x=buf, a=v):
        return lib.ltrx_norm_head_bwd_partial(P(o), P(x), P(a), P(v), P(o), P(o), 8, D, EPS, P(buf), P(ws), ctypes.byref(pr), None)

    def wgrad(D, x=buf, a=v):
        return lib.ltrx_norm_head_wgrad(P(o), P(x), P(a), P(v), P(o), P(o), 8, D, P(o), P(o), P(ws), None)

    for D in (144, 1280, 96):
        assert fwd(D) == EUNSUPPORTED and bwd(D) == EUNSUPPORTED and wgrad(D) == EUNSUPPORTED, D
    assert fwd(256, x=buf[1:]) == EUNSUPPORTED and bwd(256, x=buf[1:]) == EUNSUPPORTED          # rows not 16-byte aligned
    assert fwd(256, a=v[1:]) == EUNSUPPORTED and bwd(256, a=v[1:]) == EUNSUPPORTED
    assert wgrad(256, x=buf[1:]) == EUNSUPPORTED and wgrad(256, a=v[1:]) == EUNSUPPORTED
    assert fwd(1) == EINVAL and bwd(1) == EINVAL and wgrad(1) == EINVAL
    assert lib.ltrx_norm_head_fwd(None, P(v), P(v), P(v), P(v), 8, 256, EPS, P(o), P(o), P(o), None, None) == EINVAL
    assert lib.ltrx_norm_head_bwd_partial(P(o), P(buf), P(v), P(v), P(o), P(o), 8, 256, EPS, P(buf), P(ws), None, None) == EINVAL
    assert lib.ltrx_norm_head_bwd_workspace_bytes(0, 256) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(o).all()) and pr.value == -7 and not buf.any()                   # nothing ran


# ---------------------------------------------------------------------------------------------------------------------------------
# engine level
# ---------------------------------------------------------------------------------------------------------------------------------
def _model(d, dropout):
    from allrank_amd.model import make_model
    torch.manual_seed(5)
    return make_model(dict(sizes=[d], input_norm=False, activation=None, dropout=0.0),
                      dict(N=1, d_ff=256, h=4, positional_encoding=None, dropout=dropout), dict(d_output=1, output_activation=None), 24).to(DEV)


def _batch(lens, L=16, F=24):
    rng = np.random.default_rng(9)
    n = len(lens)
    x = rng.standard_normal((n, L, F)).astype(np.float32)
    y = rng.integers(0, 5, (n, L)).astype(np.float32)
    for i, k in enumerate(lens):
        x[i, k:], y[i, k:] = 0, -1
    return torch.tensor(x, device=DEV), torch.tensor(y, device=DEV), torch.tensor(np.asarray(lens, dtype=np.int32))


@pytest.mark.parametrize("name,compact,dropout,lens", [("padded", False, 0.0, [16, 16, 16, 16]), ("compact_ragged", True, 0.0, [16, 9, 1, 13]),
                                                       ("dropout", False, 0.1, [16, 11, 16, 5])])
def test_one_step_with_the_fused_pair_equals_the_step_without_it(name, compact, dropout, lens):
    from allrank_amd.engine import FusedTrainer
    B, L, lr = 4, 16, 1e-3
    m_on = _model(256, dropout)
    m_off = copy.deepcopy(m_on)
    x, y, hl = _batch(lens)
    kw = dict(lr=lr, use_graph=False, compact=compact, seed=3)
    on = FusedTrainer(m_on, "approxNDCGLoss", {}, B, L, **kw)
    off = FusedTrainer(m_off, "approxNDCGLoss", {}, B, L, _norm_head=False, **kw)
    assert on.norm_head and on.xf is None and not off.norm_head and off.xf is not None
    # the forward-only scorer and score() on the shared initial weights
    s_on, s_off = on.scorer(B, L, use_graph=False).run(x, y, None, lengths=hl).clone(), off.scorer(B, L, use_graph=False).run(x, y, None, lengths=hl).clone()
    assert torch.equal(s_on, s_off) and bool(s_on[y != -1].any())
    assert torch.equal(on.score(x, y, None, lengths=hl if compact else None), off.score(x, y, None, lengths=hl if compact else None))
    step = dict(lengths=hl) if compact else {}
    l_on, l_off = on.step(x, y, None, **step).clone(), off.step(x, y, None, **step).clone()
    assert torch.equal(l_on, l_off) and bool(torch.isfinite(l_on).all()), (name, l_on, l_off)
    assert torch.equal(on.scores, off.scores)
    p_off = dict(m_off.named_parameters())
    g_on, g_off = {id(r.p): r.g for r in on.params}, {id(r.p): r.g for r in off.params}
    for n_, p in m_on.named_parameters():
        assert torch.equal(g_on[id(p)], g_off[id(p_off[n_])]), (name, n_)
        assert torch.equal(p.data, p_off[n_].data), (name, n_)
    assert bool(g_on[id(m_on.output_layer.w_1.weight)].any())


def test_other_widths_keep_the_two_kernel_pair():
    from allrank_amd.engine import FusedTrainer
    x, y, _ = _batch([16, 16, 7, 16])
    ft = FusedTrainer(_model(144, 0.0), "approxNDCGLoss", {}, 4, 16, lr=1e-3, use_graph=False)
    assert not ft.norm_head and ft.xf is not None and hasattr(ft, "ws_head")
    assert bool(torch.isfinite(ft.step(x, y, None)).all())
    assert bool(ft.xf.any())                                                  # the stored LN(x) of the two-kernel path


@pytest.mark.parametrize("kw", [dict(group_wgrad=False), dict(gemm="hipblaslt")], ids=["no_group_wgrad", "hipblaslt"])
def test_configurations_without_the_deferred_reduction_keep_the_two_kernel_pair(kw):
    """the fused backward hands its (a_2, b_2) partials to the layer's ltrx_reduce_group launch; where the engine does not defer that
    reduction the step stays on ltrx_layernorm_* + ltrx_score_head_* -- and says so in ``norm_head``"""
    from allrank_amd.engine import FusedTrainer
    x, y, _ = _batch([16, 16, 7, 16])
    ft = FusedTrainer(_model(256, 0.0), "approxNDCGLoss", {}, 4, 16, lr=1e-3, use_graph=False, **kw)
    assert not ft.norm_head and ft.xf is not None
    assert bool(torch.isfinite(ft.step(x, y, None)).all())
    assert bool(ft.xf.any())
