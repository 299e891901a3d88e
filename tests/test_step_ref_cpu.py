"""tests/step_ref.py on the CPU (no GPU): (a) every fp64 reference equals the real torch operation in float64, (b) the fp32
transcription of every kernel's arithmetic is inside its bar on the inputs tests/test_gpu_step_kernels.py uses, so the bar is
attainable, and (c) every named wrong variant of a transcription is outside the bar on at least one entry of those inputs, so
the bar discriminates.  (d) measures, without asserting it, how far Adam with fp32-rounded hyperparameters is from torch's."""
import numpy as np
import pytest
import torch

from tests import step_ref as S

F = np.float32


def _same(a, b, what, scale=0.0):
    """1e-12 relative to the largest entry of the torch result (or to ``scale``, the size of the terms of a sum that cancels)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert np.abs(a - b).max() <= 1e-12 * max(np.abs(b).max(), scale, 1e-300), (what, float(np.abs(a - b).max()), float(np.abs(b).max()))


def _t64(a, rg=False):
    return torch.tensor(np.asarray(a, np.float64), requires_grad=rg)


# ---------------------------------------------------------------------------------------------------------------------------------
# (a) the references against torch, float64, Python-double hyperparameters
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decoupled", [0, 1])
def test_adam_reference_equals_torch(decoupled):
    rng = np.random.default_rng(1)
    n, lr, b1, b2, eps, wd = 257, 3e-3, 0.8, 0.95, 1e-6, 0.1
    p = _t64(rng.standard_normal(n), True)
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    pr, m, v = p.detach().numpy().copy(), np.zeros(n), np.zeros(n)
    for t in range(1, 6):
        g = rng.standard_normal(n) * 10.0 ** rng.integers(-4, 2, n)
        p.grad = _t64(g)
        opt.step()
        pr, m, v = S.adam_ref(pr, g, m, v, t, lr, b1, b2, eps, wd, decoupled, hyper=float)
        _same(pr, p.detach().numpy(), ("p", t))
        st = opt.state[p]
        _same(m, st["exp_avg"].numpy(), ("m", t))
        _same(v, st["exp_avg_sq"].numpy(), ("v", t))


@pytest.mark.parametrize("mom,nesterov,wd", [(0.0, False, 0.0), (0.9, False, 0.0), (0.9, True, 0.05)])
def test_sgd_reference_equals_torch(mom, nesterov, wd):
    rng = np.random.default_rng(2)
    n, lr = 257, 0.02
    p = _t64(rng.standard_normal(n), True)
    opt = torch.optim.SGD([p], lr=lr, momentum=mom, nesterov=nesterov, weight_decay=wd)
    pr, buf = p.detach().numpy().copy(), np.zeros(n)
    for t in range(5):
        g = rng.standard_normal(n)
        p.grad = _t64(g)
        opt.step()
        pr, bn = S.sgd_ref(pr, g, buf, lr, mom, nesterov, wd, hyper=float)
        _same(pr, p.detach().numpy(), ("p", t))
        if mom:
            buf = bn
            _same(buf, opt.state[p]["momentum_buffer"].numpy(), ("buf", t))


@pytest.mark.parametrize("case", [0, 1, 2])
def test_clip_reference_equals_torch(case):
    rng = np.random.default_rng(3)
    for (name, g, max_norm) in [S.clip_cases(rng, 255)[case]]:
        g = g.astype(np.float64)
        p = _t64(np.zeros(g.size), True)
        p.grad = _t64(g)
        total = torch.nn.utils.clip_grad_norm_([p], max_norm)
        scale, norm = S.clip_ref(g, max_norm, hyper=float)
        _same(norm, float(total), name)
        _same(g * scale, p.grad.numpy(), name)


def test_layernorm_reference_equals_torch():
    rng = np.random.default_rng(4)
    for (rows, D) in S.LN_SHAPES[:3]:
        x, wt, b, gy = S.ln_inputs(rng, rows, D)
        if rows > 2:
            x[2] = x[0][::-1]        # (not the |mean| >> std row: at 1e4 fp64 itself resolves xhat to 1e-12 only)
        ln = torch.nn.LayerNorm(D, eps=1e-5).double()
        with torch.no_grad():
            ln.weight.copy_(_t64(wt))
            ln.bias.copy_(_t64(b))
        y = ln(_t64(x))
        (y * _t64(gy)).sum().backward()
        yr, mean, rstd = S.ln_ref(x, wt, b, 1e-5, hyper=float)
        _same(yr, y.detach().numpy(), ("y", rows, D))
        dw, db = S.ln_grad_ref(x, mean, rstd, wt, gy)
        _same(dw, ln.weight.grad.numpy(), ("dw", rows, D), scale=float(np.abs(gy).max()))    # (D = 1: xhat = 0, the sum is 0)
        _same(db, ln.bias.grad.numpy(), ("db", rows, D))


def test_posenc_references_equal_torch_embedding():
    rng = np.random.default_rng(5)
    for (M, D, pad) in S.POSENC_SHAPES:
        x, table, idx, mask, dx = S.posenc_inputs(rng, M, D, pad)
        for mk in (None, mask):
            emb = torch.nn.Embedding(pad + 1, D, padding_idx=pad).double()
            with torch.no_grad():
                emb.weight.copy_(_t64(table))
            rows = torch.tensor(S.posenc_rows(idx, mk, pad))         # positional.py:44-45 clamps before the lookup
            y = 3.0 * _t64(x) + emb(rows)
            (y * _t64(dx)).sum().backward()
            _same(S.posenc_ref(x, table, idx, mk, pad, 3.0, hyper=float), y.detach().numpy(), ("y", M))
            _same(S.posenc_table_bwd_ref(dx, idx, mk, pad), emb.weight.grad.numpy(), ("dtable", M))


@pytest.mark.parametrize("kind", [1, 2])
def test_output_activation_references_equal_torch(kind):
    z, dy = S.out_act_inputs(np.random.default_rng(6))
    zt = _t64(z, True)
    y = torch.sigmoid(zt) if kind == 1 else torch.tanh(zt)
    (y * _t64(dy)).sum().backward()
    yr = S.out_act_ref(z, kind)
    _same(yr, y.detach().numpy(), "y")
    _same(S.out_act_bwd_ref(dy, yr, kind), zt.grad.numpy(), "dz")


# ---------------------------------------------------------------------------------------------------------------------------------
# (b) + (c): the transcriptions are inside the bars, the wrong variants are outside
# ---------------------------------------------------------------------------------------------------------------------------------
def _inside(got, ref, bar, what):
    r = S.worst(got, ref, bar)
    assert r <= 1.0, (what, r)


def test_adam_transcription_passes_and_mutants_fail():
    caught = {k: False for k in S.ADAM_WRONG}
    jobs = [(n, c) for n in S.ADAM_SIZES for c in S.adam_configs()] + [(S.ADAM_BIG, c) for c in S.adam_big_configs()]
    for k, (n, cfg) in enumerate(jobs):
        rng = np.random.default_rng(100 + k)
        p, g, m, v = S.adam_inputs(rng, n)
        kw = S.adam_args(cfg)
        ref, bars = S.adam_ref(p, g, m, v, **kw), S.adam_bar(p, g, m, v, **kw)
        for name, a, r, b in zip("pmv", S.adam_f32(p, g, m, v, **kw), ref, bars):
            _inside(a, r, b, (name, n, cfg))
        if n == 1027:
            for wrong in S.ADAM_WRONG:
                out = S.adam_f32(p, g, m, v, wrong=wrong, **kw)
                caught[wrong] |= any(S.over(a, r, b).any() for a, r, b in zip(out, ref, bars))
    assert all(caught.values()), caught


def test_sgd_transcription_passes_and_mutants_fail():
    caught = {k: False for k in S.SGD_WRONG}
    for k, (n, cfg) in enumerate((n, c) for n in S.SGD_SIZES for c in S.sgd_configs()):
        rng = np.random.default_rng(200 + k)
        p, g, buf = S.sgd_inputs(rng, n)
        (pr, br), (pb, bb) = S.sgd_ref(p, g, buf, **cfg), S.sgd_bar(p, g, buf, **cfg)
        pf, bf = S.sgd_f32(p, g, buf, **cfg)
        _inside(pf, pr, pb, ("p", n, cfg))
        if cfg["mom"]:
            _inside(bf, br, bb, ("buf", n, cfg))
        for wrong in S.SGD_WRONG:
            pw, bw = S.sgd_f32(p, g, buf, wrong=wrong, **cfg)
            caught[wrong] |= bool(S.over(pw, pr, pb).any() or (cfg["mom"] and S.over(bw, br, bb).any()))
    assert all(caught.values()), caught


def test_clip_transcription_passes_and_mutants_fail():
    caught = {k: False for k in S.CLIP_WRONG}
    for n in S.CLIP_SIZES:
        for (name, g, max_norm) in S.clip_cases(np.random.default_rng(300 + n % 97), n):
            ref, bar = S.clip_ref(g, max_norm), S.clip_bar(g, max_norm)
            got = S.clip_f32(g, max_norm)
            _inside(got[0], ref[0], bar[0], ("scale", name, n))
            _inside(got[1], ref[1], bar[1], ("norm", name, n))
            for wrong in S.CLIP_WRONG:
                caught[wrong] |= bool(S.over(S.clip_f32(g, max_norm, wrong=wrong)[0], ref[0], bar[0]))
    assert all(caught.values()), caught


def test_colsum_transcription_passes_and_mutants_fail():
    caught = {k: False for k in S.COLSUM_WRONG}
    for k, (M, N, ld) in enumerate(S.COLSUM_SHAPES):
        a, old = S.colsum_inputs(np.random.default_rng(400 + k), M, N)
        flat = np.full(M * ld + 8, 3.0e37, F)
        np.lib.stride_tricks.as_strided(flat, (M, N), (4 * ld, 4))[:] = a
        for acc in (0, 1):
            ref, bar = S.colsum_ref(a, old, acc), S.colsum_bar(a, old, acc)
            _inside(S.colsum_f32(flat, M, N, ld, old, acc), ref, bar, (M, N, ld, acc))
            with np.errstate(over="ignore", invalid="ignore"):
                for wrong in S.COLSUM_WRONG:
                    caught[wrong] |= bool(S.over(S.colsum_f32(flat, M, N, ld, old, acc, wrong=wrong), ref, bar).any())
    assert all(caught.values()), caught


def test_relu_bwd_transcription_passes_and_mutants_fail():
    caught = {k: False for k in S.RELU_WRONG}
    for n in S.RELU_SIZES:
        dr, r = S.relu_inputs(np.random.default_rng(500 + n % 97), n)
        assert (r == 0).any() and np.signbit(r[r == 0]).any() and (r == S.DENORM).any() and (r < 0).any()
        ref, bar = S.relu_bwd_ref(dr, r, 1.25), S.relu_bwd_bar(dr, r, 1.25)
        got = S.relu_bwd_f32(dr, r, 1.25)
        _inside(got, ref, bar, n)
        assert np.array_equal(got == 0, ref == 0) and not got[ref == 0].view(np.uint32).any()
        for wrong in S.RELU_WRONG:
            caught[wrong] |= bool(S.over(S.relu_bwd_f32(dr, r, 1.25, wrong=wrong), ref, bar).any())
    assert all(caught.values()), caught


def test_first_nonfinite_transcription_is_exact_and_mutants_fail():
    caught = {k: False for k in S.NONFINITE_WRONG}
    for n in S.NONFINITE_SIZES:
        seg = S.nonfinite_segments(n)
        base = S.nonfinite_base(np.random.default_rng(600 + n % 97), n)
        for place in S.nonfinite_placements(n, seg):
            for bad in (np.nan, np.inf, -np.inf):
                buf = base.copy()
                buf[place] = bad
                ref = S.first_nonfinite_ref(buf, seg)
                assert ref[1] == len(place) and S.first_nonfinite_f32(buf, seg) == ref, (n, place, bad)
                for wrong in S.NONFINITE_WRONG:
                    caught[wrong] |= S.first_nonfinite_f32(buf, seg, wrong=wrong) != ref
    assert all(caught.values()), caught


def test_packed_row_index_transcription_is_exact():
    for lens in S.PACKED_LENGTHS:
        cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        L = max(max(lens), 1) + 3
        assert np.array_equal(S.packed_row_index_f32(cu, L), S.packed_row_index_ref(cu, L)), lens


def test_layernorm_transcription_passes_and_mutants_fail():
    caught = {k: False for k in S.LN_WRONG}
    for k, (rows, D) in enumerate(S.LN_SHAPES):
        x, wt, b, gy = S.ln_inputs(np.random.default_rng(700 + k), rows, D)
        ref, bars = S.ln_ref(x, wt, b, 1e-5), S.ln_bar(x, wt, b, 1e-5)
        got = S.ln_f32(x, wt, b, 1e-5)
        for name, a, r, bb in zip(("y", "mean", "rstd"), got, ref, bars):
            _inside(a, r, bb, (name, rows, D))
        if D > 1:
            dwr, dbr = S.ln_grad_ref(x, got[1], got[2], wt, gy)
            dwb, dbb = S.ln_grad_bar(x, got[1], got[2], gy)
            dw, db = S.ln_grad_f32(x, got[1], got[2], gy)
            _inside(dw, dwr, dwb, ("dw", rows, D))
            _inside(db, dbr, dbb, ("db", rows, D))
        if D == 20:
            for wrong in S.LN_WRONG:
                out = S.ln_f32(x, wt, b, 1e-5, wrong=wrong)
                caught[wrong] |= bool(S.over(out[0], ref[0], bars[0]).any() and S.over(out[2], ref[2], bars[2]).any())
    assert all(caught.values()), caught


def test_posenc_transcriptions_pass_and_mutants_fail():
    caught = {("fwd", k): False for k in S.POSENC_WRONG}
    caught.update({("bwd", k): False for k in S.POSENC_BWD_WRONG})
    for k, (M, D, pad) in enumerate(S.POSENC_SHAPES):
        x, table, idx, mask, dx = S.posenc_inputs(np.random.default_rng(800 + k), M, D, pad)
        hits = np.bincount(S.posenc_rows(idx, mask, pad)[S.posenc_rows(idx, mask, pad) < pad], minlength=pad)
        assert (hits == 0).any() and (hits == 1).any() and (hits > 1).any(), (M, hits)
        for mk in (None, mask):
            ref, bar = S.posenc_ref(x, table, idx, mk, pad, 8.0), S.posenc_bar(x, table, idx, mk, pad, 8.0)
            _inside(S.posenc_f32(x, table, idx, mk, pad, 8.0), ref, bar, ("fwd", M))
            bref, bbar = S.posenc_table_bwd_ref(dx, idx, mk, pad), S.posenc_table_bwd_bar(dx, idx, mk, pad)
            got = S.posenc_table_bwd_f32(dx, idx, mk, pad)
            _inside(got, bref, bbar, ("bwd", M))
            assert not got[pad].view(np.uint32).any()
            for wrong in S.POSENC_WRONG:
                caught[("fwd", wrong)] |= bool(S.over(S.posenc_f32(x, table, idx, mk, pad, 8.0, wrong=wrong), ref, bar).any())
            for wrong in S.POSENC_BWD_WRONG:
                caught[("bwd", wrong)] |= bool(S.over(S.posenc_table_bwd_f32(dx, idx, mk, pad, wrong=wrong), bref, bbar).any())
    assert all(caught.values()), caught


def test_scale_and_output_activation_transcriptions_pass_and_mutant_fails():
    rng = np.random.default_rng(900)
    x = S.spread(rng, 1027, -20, 20)
    _inside(x * F(11.313708), S.scale_ref(x, 11.313708), S.scale_bar(x, 11.313708), "scale")
    z, dy = S.out_act_inputs(rng)
    for kind in (1, 2):
        y = S.out_act_f32(z, kind)
        _inside(y, S.out_act_ref(z, kind), S.out_act_bar(z, kind), ("fwd", kind))
        ref, bar = S.out_act_bwd_ref(dy, y, kind), S.out_act_bwd_bar(dy, y, kind)
        _inside(S.out_act_bwd_f32(dy, y, kind), ref, bar, ("bwd", kind))
        assert S.over(S.out_act_bwd_f32(dy, y, kind, z=z, wrong="at_z"), ref, bar).any(), kind


# ---------------------------------------------------------------------------------------------------------------------------------
# (d) Adam with fp32-rounded hyperparameters against torch's doubles: measured, printed, NOT asserted (include/ltrx.h quotes it)
# ---------------------------------------------------------------------------------------------------------------------------------
def test_adam_fp32_hyperparameters_deviation_from_torch_is_measured():
    rng = np.random.default_rng(7)
    n, lr, b1, b2, eps = 512, 1e-3, 0.9, 0.999, 1e-8
    sa = sb = (rng.standard_normal(n), np.zeros(n), np.zeros(n))   # two free-running (p, m, v) on the same gradients
    worst_rel = 0.0
    for t in range(1, 1001):
        g = rng.standard_normal(n)
        na = S.adam_ref(sa[0], g, sa[1], sa[2], t, lr, b1, b2, eps, 0.0, 0, hyper=S.w)
        nb = S.adam_ref(sb[0], g, sb[1], sb[2], t, lr, b1, b2, eps, 0.0, 0, hyper=float)
        ua, ub = na[0] - sa[0], nb[0] - sb[0]
        big = np.abs(ub) > 1e-2 * np.abs(ub).max()             # (relative to updates that are not themselves cancellations)
        worst_rel = max(worst_rel, float((np.abs(ua - ub)[big] / np.abs(ub)[big]).max()))
        sa, sb = na, nb
    print("largest relative difference of one Adam update, fp32-rounded against double hyperparameters, 1000 steps: %.3g" % worst_rel)
    assert np.isfinite(worst_rel)
