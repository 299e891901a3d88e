"""-m gpu: stochastic NeuralNDCG in the fused step -- FusedLoss(stochastic=True) (ltrx_neuralsort_perturb around the NeuralNDCG
kernels, ltrx_neuralsort_fold_grad behind them), its counter-based Gumbel generator, the captured FusedTrainer step and fit().

Anchors: the reference's own recorded runs (tests/golden/extra_golden.npz: draw, loss, gradient), the numpy oracle
(oracle/ltr_oracle.py::neuralndcg_stochastic) fed the draw the device used, and a numpy restatement of the generator."""
import copy
from functools import partial

import numpy as np
import pytest
import torch

from oracle import ltr_oracle as O
from tests.cases import close, grad_close, iter_stochastic_cases
from tests.test_gpu_parity import _t, _log, DEV

pytestmark = pytest.mark.gpu

NAMES = {False: "neuralNDCG", True: "neuralNDCG_transposed"}

# ---- the generator, restated (ltrx_device.h counter_hash; the dropout oracle restates the same hash for its keep decisions) ----
M32 = np.uint64(0xFFFFFFFF)
NOISE_SEED = 0x1BBCD880          # tests/test_stochastic_fused_cpu.py checks the moment bounds of 3(b) for this seed on the CPU
NOISE_SHAPE = (32, 8, 64)        # (S, B, L): 16384 draws


def _mul(a, b):
    return (a * np.uint64(b)) & M32


def hash_u32(seed, step_word, n):
    """the 32 hashed bits of elements 0 .. n-1 under ``seed ^ (step_word * 0x9E3779B9)``"""
    s = (int(seed) ^ ((int(step_word) * 0x9E3779B9) & 0xFFFFFFFF)) & 0xFFFFFFFF
    idx = np.arange(int(n), dtype=np.uint64)
    x = (idx & M32) ^ _mul(idx >> np.uint64(32), 0x9E3779B9) ^ np.uint64(s)
    x ^= x >> np.uint64(16)
    x = _mul(x, 0x85EBCA6B)
    x ^= x >> np.uint64(13)
    x = _mul(x, 0xC2B2AE35)
    x ^= x >> np.uint64(16)
    return x


def uniform_f32(seed, step_word, n):
    """U = (hash >> 8) * 2^-24, exact in fp32"""
    return (hash_u32(seed, step_word, n) >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)


def gumbel_f64(u):
    """-log(-log(U + 1e-10) + 1e-10) in fp64 from the fp32 U"""
    return -np.log(-np.log(u.astype(np.float64) + 1e-10) + 1e-10)


# ---- helpers ----
def _ragged_labels(rng, B, L):
    """labels 0..4 with a different valid length per slate (one slate full), so that the sort mask (slate i // S) and the read-out
    mask (slate i % B) of a pseudo slate differ"""
    y = rng.integers(0, 5, (B, L)).astype(np.float32)
    for b in range(1, B):
        y[b, max(1, L - (7 * b) % max(L - 1, 1) - b):] = -1
    return y


def _run(name, s, y, S, gumbel=None, seed=None, step=None, **kw):
    """one FusedLoss(stochastic=True).run; (loss, grad [B, L], draw [S, B, L], the FusedLoss)"""
    from allrank_amd import losses as E
    B, L = s.shape
    fl = E.FusedLoss(name, B, L, DEV, stochastic=True, n_samples=S, **kw)
    if gumbel is not None:
        fl.set_gumbel(_t(np.ascontiguousarray(gumbel, dtype=np.float32)))
    if seed is not None:
        fl.set_noise_key(seed, step)
    loss, grad = fl.run(_t(s), _t(y))
    torch.cuda.synchronize()
    return float(loss.item()), grad.cpu().numpy().copy(), fl.gumbel.cpu().numpy().copy(), fl


def _oracle(s, y, gum, tr, **kw):
    return O.neuralndcg_stochastic(s, y, gum, transposed=tr, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the reference's recorded runs
# ---------------------------------------------------------------------------------------------------------------------
def test_fused_stochastic_matches_reference_golden(extra_golden):
    """the 16 recorded reference runs (draw, loss, gradient) through FusedLoss with the recorded draw injected, on the automatic
    and on the general Sinkhorn kernels; same bars and strict mask as test_stochastic_neuralndcg_matches_reference_golden"""
    from allrank_amd import losses as E
    rows, bad = [], []
    for name, c, s, y, gum, rl, rg, strict in iter_stochastic_cases(extra_golden):
        kw = dict(temperature=c["tau"], k=c["k"], powered_relevancies=c["pw"], beta=c["beta"], log_scores=c["log"])
        for path in (0, 1):
            with E.neural_kernel_path(path):
                l, g, used, _ = _run(NAMES[bool(c["tr"])], s, y, gum.shape[0], gumbel=gum, **kw)
            ok = (close(l, rl) and grad_close(np.where(strict, g, 0), np.where(strict, rg, 0)) and bool(np.isfinite(g).all())
                  and np.array_equal(used, gum.astype(np.float32)))
            row = dict(case=name, path=path, loss=l, ref=float(rl), ok=bool(ok), grad_err=float(np.abs(np.where(strict, g - rg, 0)).max()),
                       grad_scale=float(np.abs(rg).max()))
            if path == 0:
                rows.append(row)
            if not ok:
                bad.append(row)
    _log("stochastic_fused_golden", rows)
    assert len(rows) == 16 and not bad, bad


# ---------------------------------------------------------------------------------------------------------------------
# 2. the oracle at shapes the fixture lacks
# ---------------------------------------------------------------------------------------------------------------------
# (name is transposed?, log_scores, k): both names, log_scores on and off, k None and 5
COMBOS = [(False, True, None), (False, False, 5), (True, True, 5), (True, False, None)]


@pytest.mark.parametrize("B,L,S", [(1, 1, 1), (3, 37, 5), (8, 64, 33), (2, 300, 4), (5, 240, 2)])
def test_fused_stochastic_matches_oracle(B, L, S):
    """loss and gradient == the oracle fed the draw the device made (read back from ``loss.gumbel``), with the dtype (fp32) and the
    bars (loss rtol 2e-5, gradient 5e-4 of its largest entry) of test_losses_match_oracle_random.  L = 300 runs the general
    Sinkhorn kernels, L = 240 the last register-resident shape, 37 and 1 the scalar (L % 4 != 0) streaming path.  With log_scores the
    batch minimum is left out of the gradient comparison (d log(s - m + 1e-10) / ds = 1e10 there, tests/cases.py)."""
    rng = np.random.default_rng(1000 * B + L + S)
    s = rng.standard_normal((B, L)).astype(np.float32)
    y = _ragged_labels(rng, B, L)
    step = torch.tensor([3], dtype=torch.int32, device=DEV)
    rows, bad = [], []
    for tr, log, k in COMBOS:
        kw = dict(k=k, log_scores=log, beta=0.1, temperature=1.0)
        l, g, gum, _ = _run(NAMES[tr], s, y, S, seed=0xC0FFEE11 + S, step=step, **kw)
        ro, rg = _oracle(s, y, gum, tr, **kw)
        strict = (s != s.min()) if log else (s == s)
        ok = (close(l, ro, rtol=2e-5) and grad_close(np.where(strict, g, 0), np.where(strict, rg, 0), rtol=5e-4)
              and bool(np.isfinite(g).all()) and bool(np.isfinite(gum).all()))
        rows.append(dict(tr=tr, log=log, k=k, loss=l, ref=float(ro), gerr=float(np.abs(np.where(strict, g - rg, 0)).max()),
                         gmax=float(np.abs(rg).max()), ok=bool(ok)))
        if not ok:
            bad.append(rows[-1])
    _log("stochastic_fused_oracle_B%d_L%d_S%d" % (B, L, S), rows)
    assert not bad, bad


def _min_cases():
    """scores [3, 37] with ragged labels; (what, scores): where the batch minimum sits decides the gradient's path through |m|"""
    rng = np.random.default_rng(5)
    B, L = 3, 37
    y = _ragged_labels(rng, B, L)
    base = rng.standard_normal((B, L)).astype(np.float32)
    out = []
    s = base.copy()
    s[0, 3] = s[1, 0] = s[2, 5] = np.float32(-4.25)
    out.append(("three tied minima, m < 0", s, 3))
    s = np.abs(base) + np.float32(1.0)
    s[0, 3] = s[1, 0] = s[2, 5] = np.float32(0.5)
    out.append(("three tied minima, m > 0", s, 3))
    s = np.abs(base) + np.float32(0.25)
    s[1, 2] = np.float32(0.0)
    out.append(("all scores >= 0, m == 0", s, 1))
    s = base.copy()
    assert y[2, L - 1] == -1
    s[2, L - 1] = np.float32(-6.5)
    out.append(("minimum in a padded slot", s, 1))
    return y, out


@pytest.mark.parametrize("tr", [False, True])
def test_fused_stochastic_gradient_through_the_batch_minimum(tr):
    """log_scores=False, EVERY element compared: the gradient's share through |min(s)| lands on all tied minima evenly with the
    sign of m (none for m == 0), also on a minimum that sits in a padded slot"""
    y, cases = _min_cases()
    step = torch.tensor([1], dtype=torch.int32, device=DEV)
    rows, bad = [], []
    for what, s, ties in cases:
        kw = dict(k=None, log_scores=False, beta=0.1)
        l, g, gum, fl = _run(NAMES[tr], s, y, 5, seed=0xA5A5F00D, step=step, **kw)
        ro, rg = _oracle(s, y, gum, tr, **kw)
        smin = fl.smin.cpu().numpy()
        ok = (close(l, ro, rtol=2e-5) and grad_close(g, rg, rtol=5e-4) and bool(np.isfinite(g).all())
              and smin[0] == s.min() and smin[1] == ties)
        rows.append(dict(what=what, loss=l, ref=float(ro), gerr=float(np.abs(g - rg).max()), gmax=float(np.abs(rg).max()),
                         g_at_min=float(g[s == s.min()][0]), ref_at_min=float(rg[s == s.min()][0]), ok=bool(ok)))
        if not ok:
            bad.append(rows[-1])
    _log("stochastic_fused_min_paths_tr%d" % tr, rows)
    assert not bad, bad


def test_fused_stochastic_all_zero_labels():
    """no slate has a relevant item: loss 0 and gradient 0 (neuralNDCG.py:66-67), both finite"""
    rng = np.random.default_rng(2)
    s = rng.standard_normal((3, 37)).astype(np.float32)
    y = np.zeros((3, 37), np.float32)
    y[1, 30:] = -1
    for tr in (False, True):
        l, g, gum, _ = _run(NAMES[tr], s, y, 5, seed=7, step=torch.zeros(1, dtype=torch.int32, device=DEV))
        assert l == 0.0 and np.isfinite(g).all() and not g.any(), (tr, l, np.abs(g).max())


@pytest.mark.parametrize("B,L,S,log,m", [(3, 37, 5, False, -2.5), (3, 37, 5, False, 0.0), (4, 64, 3, True, 1.5), (300, 1024, 2, False, 0.75)])
def test_fold_grad_contract(B, L, S, log, m):
    """ltrx_neuralsort_fold_grad alone on random pseudo-slate gradients whose sum is far from 0 (NeuralNDCG without log_scores is
    shift-invariant, so its own gradients nearly cancel in the share through |m| and the whole-loss tests above weigh that share
    lightly): == the fp64 formula with three tied minima.  300 x 1024 takes more than one round of the 256 reducing workgroups.
    Bar, worst case of the fp32 formats: 2^-24 (2 S max|term| + 32 sum|gs| / ties) -- a sum of S terms per element, then of B L
    elements through a fixed tree of depth <= 32 (<= 8 per lane, 6 + 4 per workgroup, 6 + 4 over the <= 256 partials)."""
    from allrank_amd import _lib as LB
    rng = np.random.default_rng(B + L + S)
    s = (np.abs(rng.standard_normal((B, L))) + abs(m) + 0.5).astype(np.float32)
    for b, l in ((0, 3), (B - 1, L - 1), (B // 2, 5)):
        s[b, l] = np.float32(m)
    gp = (rng.standard_normal((S * B, L)) + 0.3).astype(np.float32)
    smin = _t(np.asarray([m, 3.0], np.float32))
    out = torch.full((B, L), 7.0, device=DEV)
    ws = torch.empty(max(LB.lib().ltrx_neuralsort_stoch_workspace_bytes(B, L, S), 64), dtype=torch.uint8, device=DEV)
    st, gt = _t(s), _t(gp)
    res = []
    for _ in range(2):
        LB.check(LB.lib().ltrx_neuralsort_fold_grad(LB.ptr(gt), LB.ptr(st), LB.ptr(smin), B, L, S, int(log), LB.ptr(out), LB.ptr(ws),
                                                    LB.stream_of(out)), "fold_grad")
        res.append(out.cpu().numpy().copy())
    s64 = s.astype(np.float64)
    w = 1.0 / (s64 + abs(m) + 1e-10) if log else np.ones_like(s64)
    gs = gp.astype(np.float64).reshape(S, B, L).sum(0) * w
    ref = gs + np.where(s == np.float32(m), np.sign(m) * gs.sum() / 3.0, 0.0)
    bar = 2.0 ** -24 * (2 * S * float((np.abs(gp).reshape(S, B, L).max(0) * w).max()) + 32 * float(np.abs(gs).sum()) / 3.0)
    err = float(np.abs(res[0] - ref).max())
    _log("stochastic_fused_fold_B%d_L%d_S%d" % (B, L, S), dict(err=err, bar=bar, share=float(np.sign(m) * gs.sum() / 3.0)))
    assert err <= bar, (err, bar)
    assert np.array_equal(res[0], res[1])


# ---------------------------------------------------------------------------------------------------------------------
# 3. the generator
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def noise_runs():
    """(S, B, L) = (32, 8, 64): two runs under (NOISE_SEED, word 0) and one under word 1, same scores and labels"""
    S, B, L = NOISE_SHAPE
    rng = np.random.default_rng(11)
    s = rng.standard_normal((B, L)).astype(np.float32)
    y = _ragged_labels(rng, B, L)
    out = []
    for word in (0, 0, 1):
        out.append(_run("neuralNDCG", s, y, S, seed=NOISE_SEED, step=torch.tensor([word], dtype=torch.int32, device=DEV))[:3])
    return out


def test_device_gumbel_is_the_restated_generator(noise_runs):
    """bit-for-bit pin of the draw: device noise == fp64 evaluation of -log(-log(U + 1e-10) + 1e-10) from the same fp32 U within
    2e-6 max(1, |g|) -- two fp32 logf calls of <= 2 ulp each give about 5e-7, the bar is 4x that.  (In fp32 U + 1e-10 rounds back to
    U for U >= 2^-9, which moves g by 1e-10 / (U (-log U)): below 5e-7 while U <= 1 - 2^-12, which holds for this seed --
    tests/test_stochastic_fused_cpu.py.)"""
    S, B, L = NOISE_SHAPE
    g = noise_runs[0][2].astype(np.float64).reshape(-1)
    ref = gumbel_f64(uniform_f32(NOISE_SEED, 0, S * B * L))
    err = np.abs(g - ref) / np.maximum(1.0, np.abs(ref))
    _log("stochastic_fused_gumbel_pin", dict(max_err=float(err.max()), bar=2e-6, n=int(g.size)))
    assert g.size == 16384 and float(err.max()) <= 2e-6, float(err.max())


def test_device_gumbel_moments(noise_runs):
    """sample mean within 0.05 of Euler's constant, sample variance within 0.15 of pi^2 / 6: about 5 standard errors at n = 16384
    (variance pi^2 / 6 -> s.e. of the mean 0.010; excess kurtosis 2.4 -> s.e. of the variance 0.027)"""
    g = noise_runs[0][2].astype(np.float64).reshape(-1)
    assert abs(g.mean() - 0.5772) <= 0.05 and abs(g.var(ddof=1) - np.pi ** 2 / 6) <= 0.15, (g.mean(), g.var(ddof=1))


def test_device_gumbel_keying(noise_runs):
    """the same (seed, step word): identical bits of noise, loss and gradient; the next step word: another draw"""
    (l0, g0, n0), (l1, g1, n1), (l2, g2, n2) = noise_runs
    assert np.array_equal(n0, n1) and l0 == l1 and np.array_equal(g0, g1)
    assert float(np.mean(n0 != n2)) > 0.99 and l0 != l2
    ref = gumbel_f64(uniform_f32(NOISE_SEED, 1, n2.size))
    assert float((np.abs(n2.reshape(-1) - ref) / np.maximum(1.0, np.abs(ref))).max()) <= 2e-6


# ---------------------------------------------------------------------------------------------------------------------
# 4. the whole step
# ---------------------------------------------------------------------------------------------------------------------
def _small_model(p):
    from allrank_amd.model import make_model
    torch.manual_seed(5)
    return make_model(dict(sizes=[64], input_norm=False, activation=None, dropout=0.0),
                      dict(N=1, d_ff=128, h=2, positional_encoding=None, dropout=p), dict(d_output=1, output_activation=None), 8).to(DEV)


def _small_batch():
    rng = np.random.default_rng(21)
    B, L = 4, 24
    x = rng.standard_normal((B, L, 8)).astype(np.float32)
    y = _ragged_labels(rng, B, L)
    x[y == -1] = 0
    return _t(x), _t(y)


def test_fused_trainer_steps_with_the_stochastic_loss():
    """five captured steps (the later ones hipGraph replays): every step's loss and d loss / d scores equal the oracle's for the
    scores, labels and draw of that step, consecutive draws differ, and after the FIRST step the weights equal those of a deep copy
    stepped by the autograd Trainer with ``gumbel=`` that draw.  SGD, so that the weights after one step are linear in the gradient
    (after one Adam step they would be lr * sign(g) whatever its size); bars of test_fused_trainer_runs_the_row4_losses: 2e-5
    relative for the first step's loss, and the same for its weights."""
    from allrank_amd import losses as E
    from allrank_amd.engine import FusedTrainer, Trainer
    m1 = _small_model(0.0)
    m2 = copy.deepcopy(m1)
    x, y = _small_batch()
    B, L, S = 4, 24, 4
    args = dict(stochastic=True, n_samples=S)
    ft = FusedTrainer(m1, "neuralNDCG", args, B, L, lr=0.1, optimizer="SGD", use_graph=True, gemm="split_bf16_strict")
    ft.keep_loss_grad = True
    tr = Trainer(m2, None, torch.optim.SGD(m2.parameters(), lr=0.1))
    draws, rows = [], []
    for step in range(5):
        lf = float(ft.step(x, y).item())
        torch.cuda.synchronize()
        s, yy = ft.scores_raw.cpu().numpy().reshape(B, L).copy(), ft.y_in.cpu().numpy().copy()
        gum, g = ft.loss.gumbel.cpu().numpy().copy(), ft.loss.grad.cpu().numpy().copy()
        ro, rg = O.neuralndcg_stochastic(s, yy, gum)
        strict = s != s.min()
        rows.append(dict(step=step, loss=lf, ref=float(ro), gerr=float(np.abs(np.where(strict, g - rg, 0)).max()), gmax=float(np.abs(rg).max())))
        assert close(lf, ro, rtol=2e-5) and grad_close(np.where(strict, g, 0), np.where(strict, rg, 0), rtol=5e-4), rows[-1]
        assert all(float(np.mean(gum != d)) > 0.99 for d in draws), step
        draws.append(gum)
        if step == 0:
            tr.loss_func = partial(E.neuralNDCG, gumbel=_t(gum[..., None]), **args)
            la = float(tr.step(x, y, None).item())
            assert abs(lf - la) <= 2e-5 * (1 + abs(la)), (lf, la)
            for (n, p), q in zip(m1.named_parameters(), m2.parameters()):
                d = float((p.detach() - q.detach()).abs().max())
                assert d <= 2e-5 * (1 + float(q.detach().abs().max())), (n, d)
    assert ft.graph is not None
    _log("stochastic_fused_step", rows)


def test_fused_trainer_stochastic_loss_with_dropout_runs():
    from allrank_amd.engine import FusedTrainer
    m = _small_model(0.1)
    x, y = _small_batch()
    ft = FusedTrainer(m, "neuralNDCG_transposed", dict(stochastic=True, n_samples=4), 4, 24, lr=1e-3, use_graph=True)
    losses = [float(ft.step(x, y).item()) for _ in range(4)]
    assert np.isfinite(losses).all() and len(set(losses)) == 4, losses
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())


# ---------------------------------------------------------------------------------------------------------------------
# 5. fit()
# ---------------------------------------------------------------------------------------------------------------------
def _fit(compact, tmp_path):
    import types
    from allrank_amd import fit as EF, losses as E
    from tests.test_gpu_packed_scorer import _host_loaders, _model
    torch.manual_seed(3)
    model = _model(20, pe=dict(strategy="fixed", max_indices=200))
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    cfg = types.SimpleNamespace(metrics={"ndcg": [5, 10]}, val_metric="ndcg_5")
    tr_dl, va_dl = _host_loaders()
    res = EF.fit(epochs=1, model=model, loss_func=partial(E.neuralNDCG, stochastic=True, n_samples=4), optimizer=opt, scheduler=None,
                 train_dl=tr_dl, valid_dl=va_dl, config=cfg, gradient_clipping_norm=None, early_stopping_patience=10,
                 device=torch.device(DEV), output_dir=str(tmp_path), tensorboard_output_path=None, compact=compact)
    return res, copy.deepcopy(EF.last_run)


def test_fit_takes_the_fused_step_for_stochastic_neuralndcg(tmp_path):
    res, run = _fit(None, tmp_path)
    assert run["engine"] == "fused" and run["reason"] == "", run
    assert np.isfinite(float(res["val_metrics"]["ndcg_5"]))


def test_fit_drops_compact_for_stochastic_neuralndcg(tmp_path):
    res, run = _fit(True, tmp_path)
    assert run["engine"] == "fused" and run["compact"] is False, run


def test_sharded_fused_trainer_refuses_the_stochastic_loss():
    from allrank_amd.engine import FusedTrainer
    with pytest.raises(NotImplementedError, match="shard"):
        FusedTrainer(_small_model(0.0), "neuralNDCG", dict(stochastic=True, n_samples=4), 4, 24, force_dist=True)
