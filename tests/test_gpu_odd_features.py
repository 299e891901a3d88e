"""-m gpu: the fused step, ``score()`` and the packed scorer with an input feature count that is no multiple of 4 (MQ2007 / MQ2008
have 46 features, OHSUMED 45): the rows the first projection reads are padded to a multiple of 4 floats (engine.input_row_plan)
against a zero-padded copy of W_0, the weight gradient is taken straight off the padded rows, ``input_norm`` writes its rows into
them through ltrx_layernorm_torch_fwd_strided, and the pad job of ltrx_weight_images refreshes the padded W_0 for any column count.

One shape everywhere: 4 slates of 16 items with 16, 9, 1 and 13 valid ones, a 32-wide model with one encoder layer (4 heads,
d_ff 64), ApproxNDCG.  The references -- oracle/model_oracle.train_step in fp64, and a twin model whose features are zero-padded to
the next multiple of 4 and run through the path that existed before -- are computed once per feature count and shared."""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import ltr_oracle as O
from oracle import model_oracle as M
from tests import step_ref as S
from tests.test_gpu_gemm_contract import EINVAL, GARBAGE, Win, _libs
from tests.test_gpu_parity import DEV, _make_engine_model, _t

pytestmark = pytest.mark.gpu

B, L, H = 4, 16, 32
LENS = [16, 9, 1, 13]
FS = (1, 3, 46, 137)
STEPS = 3


def _cfg(F, norm):
    return dict(n_features=F, fc_sizes=[H], fc_activation=None, fc_input_norm=norm, N=1, d_ff=64, h=4, output_activation=None)


def _batch(F):
    rng = np.random.default_rng(100 + F)
    x = rng.standard_normal((B, L, F)).astype(np.float32)
    y = rng.integers(0, 5, (B, L)).astype(np.float32)
    for b, n in enumerate(LENS):
        y[b, n:] = -1
        x[b, n:] = 0
    return x, y


def _params(F, norm):
    p = M.init_params(_cfg(F, norm), seed=40 + F)
    if norm:                                               # (not the identity the initialisation gives: the two F-vectors matter)
        rng = np.random.default_rng(7 + F)
        p["input_layer.input_norm.weight"] = (1 + 0.2 * rng.standard_normal(F)).astype(np.float32)
        p["input_layer.input_norm.bias"] = (0.1 * rng.standard_normal(F)).astype(np.float32)
    return p


class _RecordingAdam(M.Adam):
    """model_oracle.Adam that keeps the gradients of every step it is handed"""

    def step(self, params, grads):
        self.seen = getattr(self, "seen", []) + [{k: np.array(v, np.float64) for k, v in grads.items()}]
        M.Adam.step(self, params, grads)


@functools.lru_cache(maxsize=None)
def _oracle(F, norm):
    """losses of STEPS steps and the first step's gradients of model_oracle.train_step in fp64, from the fp32 initial weights"""
    x, y = _batch(F)
    p = {k: v.astype(np.float64) for k, v in _params(F, norm).items()}
    opt = _RecordingAdam(p, lr=1e-3)
    losses = [float(M.train_step(p, _cfg(F, norm), opt, x.astype(np.float64), y, lambda s, t: O.approxndcg(s, t))[0]) for _ in range(STEPS)]
    return tuple(losses), opt.seen[0]


def _run(model, x, y, gemm, compact):
    """STEPS steps of a FusedTrainer; the losses, the first step's gradients by parameter name, and the trainer"""
    from allrank_amd.engine import FusedTrainer
    ft = FusedTrainer(model, "approxNDCGLoss", {}, B, L, lr=1e-3, gemm=gemm, compact=compact)
    xt, yt = _t(x), _t(y)
    losses, grads = [], None
    for step in range(STEPS):
        losses.append(float(ft.step(xt, yt, lengths=LENS if compact else None).item()))
        if step == 0:
            grads = {n: p.grad.detach().cpu().numpy().astype(np.float64) for n, p in model.named_parameters()}
    return losses, grads, ft


@functools.lru_cache(maxsize=None)
def _twin(F, gemm, compact):
    """the same job with the features zero-padded to the next multiple of 4 and zero columns added to W_0: the path every job took
    before.  (No such twin under input_norm: a LayerNorm over F + pad columns is another function.)"""
    F4 = (F + 3) // 4 * 4
    x, y = _batch(F)
    p = {k: v.copy() for k, v in _params(F, False).items()}
    w0 = np.zeros((H, F4), np.float32)
    w0[:, :F] = p["input_layer.layers.0.weight"]
    p["input_layer.layers.0.weight"] = w0
    x4 = np.zeros((B, L, F4), np.float32)
    x4[:, :, :F] = x
    losses, grads, _ = _run(_make_engine_model(_cfg(F4, False), p), x4, y, gemm, compact)
    grads["input_layer.layers.0.weight"] = grads["input_layer.layers.0.weight"][:, :F]
    return tuple(losses), grads


def _compare(tag, losses, grads, ref_losses, ref_grads):
    """the bars of test_fused_trainer_compact_matches_padded_and_oracle: the first loss to 1e-5 relative, later losses (two free-running
    Adam trajectories) to 2e-3, every gradient entry of the first step to 2e-5 of the largest one"""
    gscale = max(float(np.abs(g).max()) for g in ref_grads.values())
    gerr = max(float(np.abs(grads[k] - ref_grads[k]).max()) for k in ref_grads)
    print("%s: losses %r against %r; gradient error %.3g of a largest entry of %.3g" % (tag, losses, list(ref_losses), gerr, gscale))
    assert set(grads) == set(ref_grads)
    for step, (a, r) in enumerate(zip(losses, ref_losses)):
        assert np.isfinite(a) and abs(a - r) <= (1e-5 if step == 0 else 2e-3) * (1 + abs(r)), (tag, step, a, r)
    assert gerr <= 2e-5 * gscale + 1e-9, (tag, gerr, gscale)


@pytest.mark.parametrize("gemm", ["split_bf16", "hipblaslt"])
@pytest.mark.parametrize("compact", [False, True], ids=["padded", "compact"])
@pytest.mark.parametrize("F,norm", [(F, n) for F in FS for n in (False, True) if not (n and F < 2)])
def test_step_matches_the_oracle_and_the_zero_padded_twin(F, norm, compact, gemm):
    """three steps of the fused step at F features against the fp64 oracle and (without input_norm) against the zero-padded twin.
    F = 1 under input_norm is left out: a LayerNorm over one feature returns its bias for every item and the loss does not move."""
    x, y = _batch(F)
    model = _make_engine_model(_cfg(F, norm), _params(F, norm))
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    losses, grads, ft = _run(model, x, y, gemm, compact)
    assert ft._x_pad and not ft._x_large and not ft.fcstep
    assert ft.compact == compact and (compact or ft.graph is not None)         # (the padded form: the third step was a captured one)
    tag = "F %d%s %s %s" % (F, " input_norm" if norm else "", "compact" if compact else "padded", gemm)
    _compare(tag + " / oracle", losses, grads, *_oracle(F, norm))
    if not norm:
        _compare(tag + " / twin", losses, grads, *_twin(F, gemm, compact))
    assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == shapes
    assert tuple(model.input_layer.layers[0].weight.shape) == (H, F)


@pytest.mark.parametrize("gemm", ["split_bf16", "split_bf16_strict", "bf16", "hipblaslt"])
@pytest.mark.parametrize("norm", [False, True], ids=["plain", "input_norm"])
def test_pad_columns_stay_zero_through_eager_captured_and_replayed_steps(norm, gemm):
    """four steps (two eager, the capture, a replay) and a ``score()``: every pad column of the operand rows and of w0_pad is still
    zero, the features are where they were staged, and the module's parameters keep their shapes -- in all four arithmetic modes"""
    F = 46
    x, y = _batch(F)
    model = _make_engine_model(_cfg(F, norm), _params(F, norm))
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    from allrank_amd.engine import FusedTrainer
    ft = FusedTrainer(model, "approxNDCGLoss", {}, B, L, lr=1e-3, gemm=gemm)
    assert (ft._x_stride, ft._x_k, ft._x_large) == (48, 48, False) and ft.x_in.shape == (B * L, F) and ft.x_in_k.shape == (B * L, 48)
    xt, yt = _t(x), _t(y)
    modes = []
    for _ in range(4):
        before = len(ft._graphs)
        loss = ft.step(xt, yt)
        modes.append("replay" if before else ("capture" if len(ft._graphs) else "eager"))
        assert torch.isfinite(loss).all()
    assert modes == ["eager", "eager", "capture", "replay"]
    sc = ft.score(xt, yt)
    assert torch.isfinite(sc).all()
    buf = ft.x_norm_buf if norm else ft.x_in_buf
    assert buf.shape == (B * L, 48) and ft.x_in_k.data_ptr() == buf.data_ptr()
    assert not buf[:, F:].any() and torch.equal(ft.x_in, xt.reshape(B * L, F))
    assert ft.x_in.is_contiguous() == norm                    # (under input_norm the staged rows are dense: no GEMM reads them)
    if gemm != "hipblaslt":
        w0 = model.input_layer.layers[0].weight.detach()
        assert ft.w0_pad.shape == (H, 48) and not ft.w0_pad[:, F:].any() and torch.equal(ft.w0_pad[:, :F], w0)
        ref_i = torch.zeros_like(ft.w0_pad)
        ft.LB.check(ft.lib.ltrx_split_image(ft.LB.ptr(ft.w0_pad), ft.LB.ptr(ref_i), ft.w0_pad.numel(), None), "split_image")
        assert torch.equal(ft.w0_pad_i.view(torch.int32), ref_i.view(torch.int32))
    assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == shapes


@pytest.mark.parametrize("gemm", ["split_bf16", "bf16"])
@pytest.mark.parametrize("F", [46, 137])
def test_large_tile_form_at_the_smallest_batch_that_takes_it(F, gemm):
    """2048 rows (32 slates of 64) into a 256-wide FC layer: the smallest job whose input rows take the 256-float form
    (input_row_plan: large) -- the large-tile forward over K = F rounded up to 32 and the large-tile weight gradient, which reads the
    padded rows as whole tiles and keeps F of their columns.  FC + score head only, so the fp64 oracle stays cheap.  Against the oracle
    (three-product arithmetic only: the one-product mode is outside that contract) and against the zero-padded twin, which takes the
    same kernels over the same K."""
    from allrank_amd.engine import FusedTrainer
    Bl, Ll, Hl, F4 = 32, 64, 256, (F + 3) // 4 * 4
    cfg = dict(n_features=F, fc_sizes=[Hl], fc_activation=None, fc_input_norm=False, N=0, d_ff=0, h=1, output_activation=None)
    rng = np.random.default_rng(300 + F)
    x = rng.standard_normal((Bl, Ll, F)).astype(np.float32)
    y = rng.integers(0, 5, (Bl, Ll)).astype(np.float32)
    for b in range(Bl):
        n = int(rng.integers(1, Ll + 1))
        y[b, n:] = -1
        x[b, n:] = 0
    params = M.init_params(cfg, seed=60 + F)
    p4 = {k: v.copy() for k, v in params.items()}
    p4["input_layer.layers.0.weight"] = np.zeros((Hl, F4), np.float32)
    p4["input_layer.layers.0.weight"][:, :F] = params["input_layer.layers.0.weight"]
    x4 = np.zeros((Bl, Ll, F4), np.float32)
    x4[:, :, :F] = x
    out = []
    for c, p, xb in ((cfg, params, x), (dict(cfg, n_features=F4), p4, x4)):
        model = _make_engine_model(c, p)
        ft = FusedTrainer(model, "approxNDCGLoss", {}, Bl, Ll, lr=1e-3, gemm=gemm)
        assert (ft._x_stride, ft._x_k, ft._x_large) == ((F + 255) // 256 * 256, (F + 31) // 32 * 32, True) and ft.x_in.shape[1] == c["n_features"]
        losses, grads = [], None
        for step in range(STEPS):
            losses.append(float(ft.step(_t(xb), _t(y)).item()))
            if step == 0:
                grads = {n: q.grad.detach().cpu().numpy().astype(np.float64) for n, q in model.named_parameters()}
        assert not ft.x_in_buf[:, c["n_features"]:].any() and not ft.w0_pad[:, c["n_features"]:].any()
        out.append((losses, grads))
    out[1][1]["input_layer.layers.0.weight"] = out[1][1]["input_layer.layers.0.weight"][:, :F]
    tag = "large form F %d %s" % (F, gemm)
    _compare(tag + " / twin", out[0][0], out[0][1], tuple(out[1][0]), out[1][1])
    if gemm == "split_bf16":
        p64 = {k: v.astype(np.float64) for k, v in params.items()}
        opt = _RecordingAdam(p64, lr=1e-3)
        ref = [float(M.train_step(p64, cfg, opt, x.astype(np.float64), y, lambda s, t: O.approxndcg(s, t))[0]) for _ in range(STEPS)]
        _compare(tag + " / oracle", out[0][0], out[0][1], tuple(ref), opt.seen[0])


@pytest.mark.parametrize("pe", ["fixed", "learned"])
def test_positional_encoding_models_match_their_zero_padded_twin(pe):
    """the positional-encoding paths (the oracle has none): losses and first-step gradients of the padded and the compact step at 46
    features against the 48-feature twin, at the same bars"""
    from allrank_amd.engine import FusedTrainer
    from allrank_amd.model import make_model
    F, F4 = 46, 48
    x, y = _batch(F)
    x4 = np.zeros((B, L, F4), np.float32)
    x4[:, :, :F] = x
    idx = np.tile(np.arange(L, dtype=np.int64), (B, 1))
    idx[y == -1] = -1

    def build(nf):
        torch.manual_seed(11)
        return make_model(dict(sizes=[H], input_norm=False, activation=None, dropout=0.0),
                          dict(N=1, d_ff=64, h=4, positional_encoding=dict(strategy=pe, max_indices=L), dropout=0.0),
                          dict(d_output=1, output_activation=None), nf).to(DEV)

    twin, sd = build(F4), None
    with torch.no_grad():
        twin.input_layer.layers[0].weight[:, F:] = 0
        sd = {k: v.clone() for k, v in twin.state_dict().items()}
    sd["input_layer.layers.0.weight"] = sd["input_layer.layers.0.weight"][:, :F].contiguous()
    for compact in (False, True):
        out = []
        for model, xb in ((build(F), x), (copy.deepcopy(twin), x4)):
            if xb is x:
                model.load_state_dict(sd)
            ft = FusedTrainer(model, "approxNDCGLoss", {}, B, L, lr=1e-3, compact=compact)
            losses, grads = [], None
            for step in range(STEPS):
                losses.append(float(ft.step(_t(xb), _t(y), torch.tensor(idx, device=DEV), lengths=LENS if compact else None).item()))
                if step == 0:
                    grads = {n: p.grad.detach().cpu().numpy().astype(np.float64) for n, p in model.named_parameters()}
            out.append((losses, grads))
        out[1][1]["input_layer.layers.0.weight"] = out[1][1]["input_layer.layers.0.weight"][:, :F]
        _compare("pe %s %s / twin" % (pe, "compact" if compact else "padded"), out[0][0], out[0][1], tuple(out[1][0]), out[1][1])


@pytest.mark.parametrize("kind", ["plain", "input_norm", "pe_fixed"])
def test_scorer_matches_module_eval_forward_at_46_features(kind):
    """FusedScorer.run (a padded batch, host and device-counted lengths) and run_resident (straight from a resident CSR set) at 46
    features == model.eval(); model.score(), at the bar of tests/test_gpu_packed_scorer.py -- eagerly and from the captured graphs,
    with training steps moving the weights in between"""
    from allrank_amd.data import DeviceSlates
    from allrank_amd.engine import FusedTrainer
    from tests.test_gpu_packed_scorer import _bar, _model, _module_scores, _ragged
    F, Lv = 46, 40
    model = _model(F, N=1, input_norm=kind == "input_norm", pe=dict(strategy="fixed", max_indices=64) if kind == "pe_fixed" else None)
    ft = FusedTrainer(model, "approxNDCGLoss", {}, B, L, lr=1e-3)
    xt, yt, it, _ = _ragged(LENS, L, F, 1)
    lens = [40, 3, 17, 0, 39]
    x, y, idx, hl = _ragged(lens, Lv, F, 2)
    sc_ = ft.scorer(len(lens), Lv)
    valid = y != -1
    for step in range(4):
        ft.step(xt, yt, it)
        out = sc_.run(x, y, idx, lengths=hl if step % 2 else None).clone()
        ref = _module_scores(model, x, y, idx)
        assert float((sc_.scores - ref)[valid].abs().max()) <= _bar(ref, valid), (kind, step, sc_.last_mode)
        assert not out[~valid].any()
    assert sc_.last_mode in ("capture", "replay")
    buf = sc_.x_norm_buf if kind == "input_norm" else sc_.x_in_buf
    assert buf.shape[1] == 48 and not buf[:, F:].any()
    # the same slates as a resident set: items of slate q are rows q of the padded batch
    xn, yn = x.cpu().numpy(), y.cpu().numpy()
    keep = [q for q, n in enumerate(lens) if n]                        # (a resident set holds no empty slate)
    X = np.concatenate([xn[q, :lens[q]] for q in keep])
    Y = np.concatenate([yn[q, :lens[q]] for q in keep])
    ds = DeviceSlates(X, Y, np.repeat(np.arange(len(keep)), [lens[q] for q in keep]), device=DEV)
    ids = torch.arange(len(keep), dtype=torch.int64)
    res = sc_.run_resident(ds, ids, [lens[q] for q in keep]).clone()
    ref = _module_scores(model, x[keep], y[keep], idx[keep])
    v = valid[keep]
    assert torch.equal(sc_.y[:len(keep)], y[keep])
    assert float((res[:len(keep)] - ref)[v].abs().max()) <= _bar(ref, v), kind
    assert not res[:len(keep)][~v].any() and not res[len(keep):].any()
    assert not buf[:, F:].any()


# ---------------------------------------------------------------------------------------------------------------------------------
# the library additions, one call at a time
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", FS)
def test_strided_input_layernorm(D):
    """ltrx_layernorm_torch_fwd_strided against the fp64 reference and the a-priori bars tests/step_ref.py holds for nn.LayerNorm
    (ln_ref / ln_bar: the bars of ltrx_layernorm_torch_fwd), and bit for bit against that entry on dense rows; outputs prefilled with
    NaN and surrounded by it -- the pad columns of y included --, inputs surrounded by large garbage.  Row 1 is constant, row 2 has
    |mean| / std of 1e4; 37 rows: more than one block, a tail."""
    LB, lib = _libs()
    rows = 37
    x, wt, b, _ = S.ln_inputs(np.random.default_rng(900 + D), rows, D)
    ldx, ldy = D + 5, (D + 3) // 4 * 4 + 8
    X = Win((rows, D), ldx, 4, GARBAGE, x)
    Wt, Bs = Win((1, D), D, 4, GARBAGE, wt.reshape(1, D)), Win((1, D), D, 4, GARBAGE, b.reshape(1, D))
    Y, Mn, Rs = Win((rows, D), ldy), Win((1, rows), rows), Win((1, rows), rows)
    LB.check(lib.ltrx_layernorm_torch_fwd_strided(X.ptr, ldx, Wt.ptr, Bs.ptr, rows, D, 1e-5, Y.ptr, ldy, Mn.ptr, Rs.ptr, None), "strided")
    got = (Y.fetch("y"), Mn.fetch("mean")[0], Rs.fetch("rstd")[0])     # (fetch: everything outside the windows kept its sentinel)
    for name, a, r, bar in zip(("y", "mean", "rstd"), got, S.ln_ref(x, wt, b, 1e-5), S.ln_bar(x, wt, b, 1e-5)):
        worst = S.worst(a, r, bar)
        print("layernorm_torch_fwd_strided %dx%d %s: worst error / bar %.4g" % (rows, D, name, worst))
        assert worst <= 1.0, (name, worst)
    for wnd in (X, Wt, Bs):
        wnd.unchanged("strided")
    Xd = Win((rows, D), D, 4, GARBAGE, x)
    Yd, Md, Rd = Win((rows, D), D), Win((1, rows), rows), Win((1, rows), rows)
    LB.check(lib.ltrx_layernorm_torch_fwd(Xd.ptr, Wt.ptr, Bs.ptr, rows, D, 1e-5, Yd.ptr, Md.ptr, Rd.ptr, None), "dense")
    for a, d in zip(got, (Yd.fetch("y"), Md.fetch("mean")[0], Rd.fetch("rstd")[0])):
        assert np.array_equal(a.view(np.uint32), d.view(np.uint32))
    # refused before any launch: nothing is written
    Y2 = Win((rows, D), ldy)
    for kw in (dict(ldx=D - 1), dict(ldy=D - 1), dict(x=None), dict(w=None), dict(b=None), dict(y=None), dict(mean=None), dict(rstd=None),
               dict(rows=0), dict(D=0)):
        a = dict(x=X.ptr, ldx=ldx, w=Wt.ptr, b=Bs.ptr, rows=rows, D=D, y=Y2.ptr, ldy=ldy, mean=Mn.ptr, rstd=Rs.ptr)
        a.update(kw)
        rc = lib.ltrx_layernorm_torch_fwd_strided(a["x"], a["ldx"], a["w"], a["b"], a["rows"], a["D"], 1e-5, a["y"], a["ldy"], a["mean"],
                                                  a["rstd"], None)
        assert rc == EINVAL, kw
    torch.cuda.synchronize()
    assert np.isnan(Y2.fetch("refused")).all()


@pytest.mark.parametrize("cols", FS)
def test_weight_images_pad_job_takes_any_column_count(cols):
    """the pad job of ltrx_weight_images at column counts that are no multiple of 4: dst[r, :cols] = src[r, :], zeros up to the next
    multiple of 4, the columns beyond untouched, and the image == ltrx_split_image of that -- in fp32 copy and image alike.  37 rows of
    an ld of cols rounded up to 4 plus 8; NaN prefill and guards; bad strides and null pointers refused with nothing written."""
    LB, lib = _libs()
    rows, c4 = 37, (cols + 3) // 4 * 4
    ld = c4 + 8
    rng = np.random.default_rng(950 + cols)
    nflat = 64
    flat = _t(rng.standard_normal(nflat).astype(np.float32))
    flat_i = torch.zeros(nflat, device=DEV)
    src = Win((rows, cols), cols, 4, GARBAGE, (rng.standard_normal((rows, cols)) * 2.0 ** rng.integers(-20, 21, (rows, 1))).astype(np.float32))
    dst, img = Win((rows, ld), ld), Win((rows, ld), ld)

    def call(s=src.ptr, r=rows, c=cols, l=ld, d=dst.ptr, i=img.ptr):
        return lib.ltrx_weight_images(LB.ptr(flat), nflat, LB.ptr(flat_i), None, None, None, None, 0, 0, s, r, c, l, d, i, None)

    odd = lambda w: ctypes.c_void_p(w.ptr.value + 4)          # noqa: E731
    for kw in (dict(l=cols), dict(l=c4 - 4), dict(l=c4 + 2), dict(l=0), dict(d=None), dict(i=None), dict(r=0), dict(c=0), dict(s=odd(src)),
               dict(d=odd(dst)), dict(i=odd(img))):
        assert call(**kw) == EINVAL, kw
    torch.cuda.synchronize()
    assert np.isnan(dst.fetch("refused")).all() and np.isnan(img.fetch("refused")).all()
    LB.check(call(), "weight_images(pad job)")
    got, got_i = dst.fetch("dst"), img.fetch("image")
    want = np.full((rows, ld), np.nan, np.float32)
    want[:, :c4] = 0
    want[:, :cols] = src.view(src.host)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    ref_in = torch.zeros((rows, c4), device=DEV)
    ref_in[:, :cols] = _t(src.view(src.host).copy())
    ref_i = torch.zeros_like(ref_in)
    LB.check(lib.ltrx_split_image(LB.ptr(ref_in), LB.ptr(ref_i), ref_in.numel(), None), "split_image")
    assert np.array_equal(got_i[:, :c4].view(np.uint32), ref_i.cpu().numpy().view(np.uint32)) and np.isnan(got_i[:, c4:]).all()
    src.unchanged("src")


def test_unsupported_widths_are_refused_in_the_constructor():
    """a hidden width that is no multiple of 4, or a head width the attention kernels refuse, raises NotImplementedError -- naming the
    width -- before the trainer touches the module, so fit() falls back to the autograd Trainer instead of dying in its first batch"""
    from allrank_amd.engine import FusedTrainer
    from allrank_amd.model import make_model

    def build(sizes, h, F=46):
        return make_model(dict(sizes=sizes, input_norm=False, activation=None, dropout=0.0),
                          dict(N=1, d_ff=64, h=h, positional_encoding=None, dropout=0.0), dict(d_output=1, output_activation=None), F).to(DEV)

    for sizes, h, word in (([50], 5, "50"), ([36], 6, "36 / 6"), ([40], 4, "40 / 4"), ([32, 30, 32], 4, "30")):
        model = build(sizes, h)
        ptrs = [p.data_ptr() for p in model.parameters()]
        with pytest.raises(NotImplementedError, match=word):
            FusedTrainer(model, "approxNDCGLoss", {}, B, L)
        assert [p.data_ptr() for p in model.parameters()] == ptrs and all(p.grad is None for p in model.parameters())
    # d_model 36 with 3 heads is NOT such a width: d_k = 12 is a multiple of 4, ltrx_mha_fwd / ltrx_mha_bwd take it (their contract
    # test pins d_k = 4), and the step ran it before feature counts were freed.  It keeps running, at 46 features too, and follows the
    # fp64 oracle at the step bars above.
    cfg = dict(_cfg(46, False), fc_sizes=[36], h=3)
    params = M.init_params(cfg, seed=3)
    x, y = _batch(46)
    p64 = {k: v.astype(np.float64) for k, v in params.items()}
    opt = _RecordingAdam(p64, lr=1e-3)
    ref = [float(M.train_step(p64, cfg, opt, x.astype(np.float64), y, lambda s, t: O.approxndcg(s, t))[0]) for _ in range(STEPS)]
    losses, grads, _ = _run(_make_engine_model(cfg, params), x, y, "split_bf16", False)
    _compare("d_model 36, h 3 / oracle", losses, grads, tuple(ref), opt.seen[0])


def test_sharded_step_at_46_features_equals_the_plain_step():
    """the sharded form (flat layout and gradient buckets unchanged) on a one-rank nccl group, in a process of its own:
    tests/odd_features_dist_worker.py"""
    import os
    import subprocess
    import sys
    from allrank_amd.launch import free_port
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port()), HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "odd_features_dist_worker.py")], env=env, capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0 and "ODD_FEATURES_DIST_OK" in r.stdout, (r.stdout[-3000:], r.stderr[-4000:])
