"""-m gpu: FusedTrainer(compact="graph") -- the variable-length training step at bucketed row counts, captured and replayed per
row bucket -- and its one new kernel, ltrx_zero_rows_cu.

The model is the one of test_fused_trainer_compact_matches_padded_and_oracle (F 20, FC [32], N 2, d_ff 64, h 4); B 6, L 70 (420
slots, buffers of 448 rows: buckets 32 ... 256, 288, 320, ...) and B 5, L 70 where B * L must be no multiple of 32."""
import copy
import itertools
import types
from functools import partial

import numpy as np
import pytest
import torch

from oracle import ltr_oracle as O
from oracle import model_oracle as M
from tests.golden import make_call_trace_fixture as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F, L = 20, 70
CFG = dict(n_features=F, fc_sizes=[32], fc_activation=None, fc_input_norm=False, N=2, d_ff=64, h=4, output_activation=None)


def _model(dropout=0.0, pe=None, d_output=1, params=None):
    from allrank_amd.model import make_model
    torch.manual_seed(21)
    model = make_model(dict(sizes=[32], input_norm=False, activation=None, dropout=0.0),
                       dict(N=2, d_ff=64, h=4, positional_encoding=pe, dropout=dropout), dict(d_output=d_output, output_activation=None), F)
    if params is not None:
        model.load_state_dict({k: torch.tensor(v) for k, v in params.items()}, strict=True)
    return model.to(DEV)


def _lens(n, B, seed, lo=0):
    """B slate lengths in [lo, L] that sum to n (lo = 0: empty slates happen)"""
    rng = np.random.default_rng(seed)
    lens = [n // B] * B
    lens[0] += n - sum(lens)
    for _ in range(24):
        i, j = (int(v) for v in rng.integers(0, B, 2))
        if i != j:
            d = int(rng.integers(0, min(lens[i] - lo, L - lens[j]) + 1))
            lens[i], lens[j] = lens[i] - d, lens[j] + d
    assert sum(lens) == n and all(lo <= k <= L for k in lens)
    return lens


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def _same_bits(a, b, what):
    la, lb = a.loss.loss, b.loss.loss
    assert torch.equal(_bits(la), _bits(lb)), (what, "loss", float(la), float(lb))
    assert torch.equal(_bits(a.flat_g), _bits(b.flat_g)), (what, "flat_g", float((a.flat_g - b.flat_g).abs().max()))
    assert torch.equal(_bits(a.flat_p), _bits(b.flat_p)), (what, "flat_p", float((a.flat_p - b.flat_p).abs().max()))


def _twins(B, loss="approxNDCGLoss", largs=None, dropout=0.0, pe=None, second=None, **kw):
    """two trainers from the same weights: compact="graph" captured, and ``second`` (default: the same mode run eagerly)"""
    from allrank_amd.engine import FusedTrainer
    m1 = _model(dropout, pe)
    m2 = copy.deepcopy(m1)
    a = FusedTrainer(m1, loss, largs or {}, B, L, lr=1e-3, compact="graph", use_graph=True, seed=77, **kw)
    b = FusedTrainer(m2, loss, largs or {}, B, L, lr=1e-3, seed=77, **dict(second or dict(compact="graph", use_graph=False), **kw))
    return a, b


# ------------------------------------------------------------------------------------------------------------------
# 1. replay == eager, bit for bit
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dropout", [0.0, 0.1])
def test_replay_equals_eager_bit_for_bit(dropout):
    """two trainers from the same weights, one replaying and one running the same launch sequence eagerly, over 12 batches that visit
    three row buckets four times each, interleaved: loss, gradients and weights equal as bits at every step (with dropout too: the
    step word lives on the device), per bucket eager, eager, capture, replay.  (Before the mode existed ``compact="graph"`` was just
    truthy: nothing was captured and there was no ``last_mode``.)"""
    B = 6
    ft, fe = _twins(B, dropout=dropout)
    assert ft.compact is True and ft.compact_graph is True and fe.compact is True and fe.compact_graph is True
    assert ft.use_graph and not fe.use_graph and ft.max_graphs == 8
    counts = {192: [180, 170, 192, 161], 256: [240, 230, 250, 256], 288: [270, 260, 288, 257]}
    assert ft.bucket_of([n for ns in counts.values() for n in ns]) == [192] * 4 + [256] * 4 + [288] * 4
    modes = {b: [] for b in counts}
    for visit in range(4):
        for bucket in (192, 256, 288):                              # interleaved
            n = counts[bucket][visit]
            x, y, _, hl = G._batch(_lens(n, B, 100 * visit + bucket), L, F, 10 * visit + bucket)
            lengths = hl if (visit + bucket // 32) % 2 else None    # host lengths, or counted on the device
            ft.step(x, y, lengths=lengths)
            fe.step(x, y, lengths=lengths)
            assert ft.rows == fe.rows == bucket and ft.n_valid == fe.n_valid == n
            assert fe.last_mode == "eager"
            modes[bucket].append(ft.last_mode)
            _same_bits(ft, fe, (bucket, visit))
            assert torch.equal(ft.scores, fe.scores) and bool(torch.isfinite(ft.loss.loss).all())
    assert all(m == ["eager", "eager", "capture", "replay"] for m in modes.values()), modes
    assert len(ft._graphs) == 3 and sorted(k[2] for k in ft._graphs) == [192, 256, 288]
    assert dict(ft.bucket_counts) == {192: 4, 256: 4, 288: 4}
    assert ft.mode_counts == {"eager": 6, "capture": 3, "replay": 3}
    # set_lr drops the captures and keeps the warm-up counts: the next visit of a bucket records again
    ft.set_lr(5e-4)
    fe.set_lr(5e-4)
    assert len(ft._graphs) == 0
    x, y, _, hl = G._batch(_lens(245, B, 5), L, F, 6)
    ft.step(x, y, lengths=hl)
    fe.step(x, y, lengths=hl)
    assert ft.last_mode == "capture" and ft.rows == 256
    _same_bits(ft, fe, "after set_lr")


# ------------------------------------------------------------------------------------------------------------------
# 2. against compact=True, the padded step and the fp64 oracle
# ------------------------------------------------------------------------------------------------------------------
CASES = {
    "approxNDCGLoss": ("approxNDCGLoss", {}, lambda s, t: O.approxndcg(s, t)),
    "listNet": ("listNet", {}, lambda s, t: O.listnet(s, t)),
    "lambdaLoss": ("lambdaLoss", dict(weighing_scheme="ndcgLoss2_scheme"), lambda s, t: O.lambdaloss(s, t, weighing_scheme="ndcgLoss2_scheme")),
    "rankNet": ("rankNet", {}, lambda s, t: O.ranknet(s, t)),
    # (the model oracle restates d_output == 1 without a positional encoding: these two are held to the two engine steps)
    "ordinal": ("ordinal", {"n": 4}, None),
    "learned_pe": ("listNet", {}, None),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_matches_compact_padded_and_oracle(case):
    """the bars of test_fused_trainer_compact_matches_padded_and_oracle; the batch changes its lengths every step (all in the
    256-row bucket, so the four steps are eager, eager, capture, replay)"""
    from allrank_amd.engine import FusedTrainer
    loss_name, largs, ofn = CASES[case]
    B = 6
    pe = dict(strategy="learned", max_indices=100) if case == "learned_pe" else None
    params = M.init_params(CFG, seed=21) if ofn is not None else None
    m_g = _model(0.0, pe, 4 if case == "ordinal" else 1, params)
    m_c, m_p = copy.deepcopy(m_g), copy.deepcopy(m_g)
    fg = FusedTrainer(m_g, loss_name, largs, B, L, lr=1e-3, compact="graph")
    fc = FusedTrainer(m_c, loss_name, largs, B, L, lr=1e-3, compact=True)
    fp = FusedTrainer(m_p, loss_name, largs, B, L, lr=1e-3, use_graph=False)
    oopt = M.Adam(params, lr=1e-3) if ofn is not None else None
    rows, modes = [], []
    for step, n in enumerate([230, 250, 241, 256]):
        lens = _lens(n, B, 30 + step, lo=1)                         # (the oracle's attention, like the reference's, has no value for a
        x, y, idx, hl = G._batch(lens, L, F, 40 + step)             #  slate without items; the bit-for-bit tests cover empty slates)
        kw = dict(indices=idx) if pe else {}
        lg = float(fg.step(x, y, lengths=hl if step % 2 else None, **kw).item())
        refs = [float(fc.step(x, y, lengths=hl, **kw).item()), float(fp.step(x, y, **kw).item())]
        if ofn is not None:
            refs.append(float(M.train_step(params, CFG, oopt, x.cpu().numpy(), y.cpu().numpy(), ofn)[0]))
        modes.append(fg.last_mode)
        rows.append((lg, refs))
        print(case, "step", step, "graph", lg, "compact / padded / oracle", refs)
        tol = 1e-5 if step == 0 else 2e-3
        assert all(abs(lg - r) <= tol * (1 + abs(r)) for r in refs), rows
        if step == 0:
            assert fg.n_valid == n and fg.rows == 256
            v = (y != -1)
            for ref in (fc, fp):
                gscale = float(ref.flat_g.abs().max().item())
                gerr = float((fg.flat_g - ref.flat_g).abs().max().item())
                serr = float((fg.scores[v] - ref.scores[v]).abs().max().item())
                print(case, "first-step gradient error", gerr, "of", gscale, "score error", serr)
                assert gerr <= 2e-5 * gscale + 1e-9, (gerr, gscale)
                assert serr < 2e-5
            assert float(fg.scores[~v].abs().max().item()) == 0.0        # padded slots: 0, as compact training leaves them
    assert modes == ["eager", "eager", "capture", "replay"]
    for ref in (m_c, m_p):
        sd1, sd2 = m_g.state_dict(), ref.state_dict()
        for k in sd1:
            assert (sd1[k] - sd2[k]).abs().max().item() <= 8.1e-3, k


# ------------------------------------------------------------------------------------------------------------------
# 3. alignment rows carry nothing
# ------------------------------------------------------------------------------------------------------------------
def _poison_alignment_rows(ft):
    """NaN into rows n_valid .. of every row-major activation and gradient buffer (the _alloc_forward set, the backward's)"""
    bufs = [ft.x_in, ft.scores_c, ft.xsum_f, ft.xf, ft.mean_f, ft.rstd_f, ft.dsc_c, ft.d_r, ft.dqkv, ft.d_o, ft.tmp_d, ft.d_br, ft.d_a,
            ft.d_b, getattr(ft, "d_c", None), getattr(ft, "x_pe", None)] + list(ft.fc_out) + list(ft.fc_dgrad)
    for st in ft.layers:
        bufs += [st[k] for k in ("xsum0", "xn0", "mean0", "rstd0", "xn1", "mean1", "rstd1", "qkv", "o", "x1", "r")]
    seen = 0
    for t in bufs:
        if t is not None:
            assert t.shape[0] == ft.cap
            t[ft.n_valid:] = float("nan")
            seen += 1
    return seen


def test_alignment_rows_carry_nothing():
    B, n = 6, 257                                                   # one above the 256 rung: 31 alignment rows, the most this ladder
    ft, tw = _twins(B, loss="listNet", dropout=0.1, second=dict(compact="graph", use_graph=True))      # has below 512 rows
    modes = []
    for step in range(5):
        x, y, _, hl = G._batch(_lens(n, B, 60 + step), L, F, 70 + step)
        if step in (0, 4):                                          # before an eager step, before a replay
            ft.n_valid = n
            assert _poison_alignment_rows(ft) >= 30
        ft.step(x, y, lengths=hl)
        tw.step(x, y, lengths=hl)
        modes.append(ft.last_mode)
        assert ft.rows == 288 and ft.rows - ft.n_valid == 31
        assert bool(torch.isfinite(ft.loss.loss).all()) and bool(torch.isfinite(ft.flat_g).all()) and bool(torch.isfinite(ft.flat_p).all())
        _same_bits(ft, tw, step)
        # what the step left in the alignment rows a later kernel reads: zeros where a slate-wise kernel skipped them
        for st in ft.layers:
            assert float(st["o"][n:ft.rows].abs().max()) == 0.0
        assert float(ft.dqkv[n:ft.rows].abs().max()) == 0.0 and float(ft.dsc_c[n:ft.rows].abs().max()) == 0.0
    assert modes == ["eager", "eager", "capture", "replay", "replay"]


# ------------------------------------------------------------------------------------------------------------------
# 4. ladder ends
# ------------------------------------------------------------------------------------------------------------------
def test_one_valid_item():
    ft, fc = _twins(6, loss="listNet", second=dict(compact=True))
    x, y, _, hl = G._batch([0, 0, 1, 0, 0, 0], L, F, 3)
    for lengths in (hl, None, hl):
        lg, lc = float(ft.step(x, y, lengths=lengths).item()), float(fc.step(x, y, lengths=hl).item())
        assert ft.rows == 32 and ft.n_valid == 1 and np.isfinite(lg) and abs(lg - lc) <= 1e-5 * (1 + abs(lc))
        assert bool(torch.isfinite(ft.flat_p).all())
        assert float((ft.flat_g - fc.flat_g).abs().max()) <= 2e-5 * float(fc.flat_g.abs().max()) + 1e-9
    assert ft.last_mode == "capture"
    with pytest.raises(ValueError, match="no valid item"):
        ft.step(x, torch.full_like(y, -1.0))


def test_every_slot_valid_runs_the_rows_allocated():
    from allrank_amd.engine import row_bucket
    B = 5                                                           # 350 slots: no multiple of 32
    ft, fp = _twins(B, second=dict(use_graph=False))
    assert ft.cap == 352 == row_bucket(350, 352) and ft.M == 350
    sized = [ft.x_in, ft.scores_c, ft.dsc_c, ft.dqkv, ft.d_a, ft.idx] + [st["o"] for st in ft.layers]
    assert all(t.shape[0] == ft.cap for t in sized)
    for step in range(4):
        x, y, _, hl = G._batch([L] * B, L, F, 80 + step)
        lg, lp = float(ft.step(x, y, lengths=hl if step else None).item()), float(fp.step(x, y).item())
        assert ft.n_valid == 350 and ft.rows == 352 <= ft.cap
        tol = 1e-5 if step == 0 else 2e-3
        assert abs(lg - lp) <= tol * (1 + abs(lp)), (step, lg, lp)
        if step == 0:
            assert float((ft.flat_g - fp.flat_g).abs().max()) <= 2e-5 * float(fp.flat_g.abs().max()) + 1e-9
            assert float((ft.scores - fp.scores).abs().max()) < 2e-5
    assert ft.last_mode == "replay"


def test_short_last_batch_in_a_warm_bucket_is_captured_on_its_first_visit():
    from allrank_amd.engine import pad_batch
    B = 6
    ft, fe = _twins(B, loss="listNet")
    seen = []
    for step, (slates, n) in enumerate([(6, 240), (6, 250), (6, 230), (4, 235), (4, 245), (6, 256)]):
        x, y, idx, hl = G._batch(_lens(n, slates, 90 + step), L, F, 95 + step)
        x, y, idx = pad_batch(x, y, idx, B)                          # the short batch: topped up with fully padded slates
        hl = torch.cat([hl, hl.new_zeros(B - slates)])
        for t in (ft, fe):
            t.step(x, y, global_batch=slates, lengths=hl)
        seen.append((ft.last_mode, ft.rows))
        _same_bits(ft, fe, step)
    assert seen == [("eager", 256), ("eager", 256), ("capture", 256), ("capture", 256), ("replay", 256), ("replay", 256)]
    assert sorted(ft._graphs) == [(4.0, True, 256), (6.0, True, 256)]


# ------------------------------------------------------------------------------------------------------------------
# 5. a replayed step makes no library call besides staging
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_pe", [False, True])
def test_a_replayed_step_calls_the_library_for_staging_only(with_pe):
    from allrank_amd.engine import FusedTrainer
    B = 6
    with G.proxied() as proxy:
        model = _model(0.1, dict(strategy="learned", max_indices=100) if with_pe else None)
        ft = FusedTrainer(model, "listNet", {}, B, L, lr=1e-3, compact="graph", seed=5)
        names = []
        for step in range(4):
            x, y, idx, hl = G._batch(_lens(200 + step, B, step), L, F, step)
            proxy.log = []
            try:
                ft.step(x, y, indices=idx if with_pe else None, lengths=hl)
            finally:
                names.append([c[0] for c in proxy.log])
                proxy.log = None
            torch.cuda.synchronize()
        assert ft.last_mode == "replay"
    assert names[3] == ["ltrx_ingest_batch"] + ["ltrx_gather_rows_cu"] * (2 if with_pe else 1), names[3]
    # ... where an eager step of the mode makes them all -- the device-count forms, and never the host-count ones
    assert len(names[0]) > 40 and {"ltrx_zero_rows_cu", "ltrx_scatter_rows_cu", "ltrx_mha_fwd", "ltrx_mha_bwd", "ltrx_adam_step"} <= set(names[0])
    assert names[0].count("ltrx_zero_rows_cu") == 4                  # o and dqkv of two layers
    assert not {"ltrx_gather_rows", "ltrx_scatter_rows", "ltrx_packed_row_index"} & set(names[0])


# ------------------------------------------------------------------------------------------------------------------
# 6. ltrx_zero_rows_cu
# ------------------------------------------------------------------------------------------------------------------
def test_zero_rows_cu_zeroes_the_tail_rows_and_nothing_else():
    from allrank_amd import _lib as LB
    lib = LB.lib()
    B, guard = 3, 64
    for rows, tail_from, cols, ld, off in itertools.product((32, 96), (0, 5, "rows", "rows+3"), (1, 4, 128, 130), (130, 132), (0, 1, 4)):
        n = {"rows": rows, "rows+3": rows + 3}.get(tail_from, tail_from)
        flat = torch.full((guard + off + rows * ld + guard,), 7.0, device=DEV)
        x = flat[guard + off:guard + off + rows * ld].view(rows, ld)
        assert (x.data_ptr() % 16 == 0) == (off % 4 == 0)
        cu = torch.tensor([0, n // 3, n // 3, n], dtype=torch.int32, device=DEV)
        want = flat.clone()
        want[guard + off:guard + off + rows * ld].view(rows, ld)[min(n, rows):, :cols] = 0.0
        rc = lib.ltrx_zero_rows_cu(LB.ptr(x), ld, cols, LB.ptr(cu), B, rows, LB.stream_of(x))
        assert rc == 0 and torch.equal(flat, want), (rows, n, cols, ld, off)
        if n >= rows:
            assert bool((flat == 7.0).all())
    # invalid arguments: the status, and not one write
    flat = torch.full((2 * guard + 32 * 132,), 7.0, device=DEV)
    x = flat[guard:guard + 32 * 132].view(32, 132)
    cu = torch.zeros(B + 1, dtype=torch.int32, device=DEV)
    st = LB.stream_of(x)
    bad = [(None, 132, 4, LB.ptr(cu), B, 32), (LB.ptr(x), 132, 4, None, B, 32), (LB.ptr(x), 132, 4, LB.ptr(cu), 0, 32),
           (LB.ptr(x), 132, 4, LB.ptr(cu), B, 0), (LB.ptr(x), 132, 4, LB.ptr(cu), B, -32), (LB.ptr(x), 132, 0, LB.ptr(cu), B, 32),
           (LB.ptr(x), 0, 4, LB.ptr(cu), B, 32), (LB.ptr(x), 128, 132, LB.ptr(cu), B, 32), (LB.ptr(x), 132, -4, LB.ptr(cu), -B, 32)]
    for args in bad:
        assert lib.ltrx_zero_rows_cu(*args, st) == -1, args[1:3] + args[4:]
    torch.cuda.synchronize()
    assert bool((flat == 7.0).all())


# ------------------------------------------------------------------------------------------------------------------
# 7. refusals
# ------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from allrank_amd.engine import FusedTrainer
    model = _model()
    before = [(p.data_ptr(), p.grad) for p in model.parameters()]
    with pytest.raises(NotImplementedError, match="sharding"):
        FusedTrainer(model, "listNet", {}, 6, L, compact="graph", force_dist=True)
    assert [(p.data_ptr(), p.grad) for p in model.parameters()] == before        # refused before any parameter was re-pointed
    with pytest.raises(ValueError, match="compact"):
        FusedTrainer(model, "listNet", {}, 6, L, compact="packed")
    assert [(p.data_ptr(), p.grad) for p in model.parameters()] == before
    ft = FusedTrainer(model, "listNet", {}, 6, L, compact="graph")
    x, y, _, hl = G._batch(_lens(200, 6, 1), L, F, 2)
    k = int(hl.argmax())
    y[k, 1], x[k, 1] = -1.0, 0.0                                    # padding between the valid items of one slate
    with pytest.raises(ValueError, match="valid items first"):
        ft.step(x, y)
    y[k, 1] = 2.0
    assert np.isfinite(float(ft.step(x, y).item()))                 # (the same trainer goes on with a well-formed batch)
    st = FusedTrainer(_model(), "neuralNDCG", dict(stochastic=True), 6, L, compact="graph")
    assert st.compact_graph is False and st.compact is False
    fcm = G._model(F, [32])                                         # FCModel([32]) -> OutputLayer + listNet: the slate-resident step
    fs = FusedTrainer(fcm, "listNet", {}, 6, L, compact="graph")
    assert fs.fcstep and fs.compact_graph is False and fs.compact is False


# ------------------------------------------------------------------------------------------------------------------
# 8. fit(compact="graph") and ALLRANK_AMD_COMPACT
# ------------------------------------------------------------------------------------------------------------------
def _fit(compact, tmp_path, loss=None, epochs=4):
    from allrank_amd import losses as E, fit as EF
    from tests.test_gpu_fit import _loaders, _model as fit_model
    cfg = types.SimpleNamespace(metrics={"ndcg": [5]}, val_metric="ndcg_5")
    train_dl, val_dl = _loaders(n_train=40, n_val=24, L=30, F=20, bs=16)          # 16 / 16 / 8 slates per epoch, ragged
    model = fit_model(20)
    res = EF.fit(epochs=epochs, model=model, loss_func=loss or partial(E.approxNDCGLoss, alpha=1.0),
                 optimizer=torch.optim.Adam(model.parameters(), lr=2e-3), scheduler=None, train_dl=train_dl, valid_dl=val_dl, config=cfg,
                 gradient_clipping_norm=None, early_stopping_patience=10, device=torch.device(DEV), output_dir=str(tmp_path),
                 tensorboard_output_path=None, compact=compact)
    return res, dict(EF.last_run)


def test_fit_compact_graph_and_the_environment_variable(tmp_path, monkeypatch):
    monkeypatch.delenv("ALLRANK_AMD_COMPACT", raising=False)
    ref_res, ref = _fit(True, tmp_path)
    assert ref["compact"] is True and ref["compact_graph"] is None and ref["compact_graph_reason"] == ""
    res, run = _fit("graph", tmp_path)
    assert run["engine"] == "fused" and run["compact"] is True and run["compact_graph_reason"] == ""
    cg = run["compact_graph"]
    assert set(cg) == {"buckets", "captures", "replays", "eager_steps", "evictions"}
    assert cg["replays"] > 0 and cg["captures"] > 0 and cg["evictions"] == 0
    assert cg["captures"] + cg["replays"] + cg["eager_steps"] == sum(cg["buckets"].values()) == 12
    assert all(b % 32 == 0 for b in cg["buckets"])
    for e_g, e_c in zip(run["epoch_log"], ref["epoch_log"]):
        print("val_loss graph", e_g["val_loss"], "compact", e_c["val_loss"])
        assert abs(e_g["val_loss"] - e_c["val_loss"]) <= 2e-3 * (1 + abs(e_c["val_loss"])), (e_g, e_c)
    assert abs(float(res["train_metrics"]["ndcg_5"]) - float(ref_res["train_metrics"]["ndcg_5"])) <= 2e-3
    monkeypatch.setenv("ALLRANK_AMD_COMPACT", "graph")              # what an unmodified main.py can say
    _, env = _fit(None, tmp_path)
    assert env["compact"] is True and env["compact_graph"] == cg
    assert [e["val_loss"] for e in env["epoch_log"]] == [e["val_loss"] for e in run["epoch_log"]]
    monkeypatch.setenv("ALLRANK_AMD_COMPACT", "yes")
    with pytest.raises(ValueError, match="ALLRANK_AMD_COMPACT"):
        _fit(None, tmp_path, epochs=1)


def test_fit_says_why_the_mode_does_not_apply(tmp_path):
    from allrank_amd import losses as E
    _, run = _fit("graph", tmp_path, loss=partial(E.neuralNDCG, stochastic=True), epochs=1)
    assert run["engine"] == "fused" and run["compact_graph"] is None and "stochastic" in run["compact_graph_reason"]
