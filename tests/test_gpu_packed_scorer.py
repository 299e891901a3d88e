"""-m gpu: the packed, captured forward-only validation scorer (engine.FusedScorer, fit(val_scorer="packed")) and its device-count
pack / unpack kernels (ltrx_assemble_packed, ltrx_gather_rows_cu, ltrx_scatter_rows_cu) -- validation slates longer than the
training slates, as the reference pads every non-training role to its longest slate (dataset_loading.py:185-194,212-227)."""
import copy
import types
from functools import partial

import numpy as np
import pytest
import torch

from oracle import model_oracle as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _model(F, d=32, h=4, N=2, d_ff=64, pe=None, input_norm=False, act=None, out_act=None, d_output=1, dropout=0.1, sizes=None):
    from allrank_amd.model import make_model
    torch.manual_seed(7)
    tr = dict(N=N, d_ff=d_ff, h=h, positional_encoding=pe, dropout=dropout) if N else None
    return make_model(dict(sizes=sizes or [d], input_norm=input_norm, activation=act, dropout=0.0), tr,
                      dict(d_output=d_output, output_activation=out_act), F).to(DEV)


def _ragged(lens, L, F, seed):
    """padded batch (valid items first, features 0 / labels -1 / indices -1 on padding) with the given slate lengths"""
    rng = np.random.default_rng(seed)
    n = len(lens)
    x = rng.standard_normal((n, L, F)).astype(np.float32)
    y = rng.integers(0, 5, (n, L)).astype(np.float32)
    idx = np.tile(np.arange(L, dtype=np.int64), (n, 1))
    for b, k in enumerate(lens):
        x[b, k:], y[b, k:], idx[b, k:] = 0, -1, -1
    return (torch.tensor(x, device=DEV), torch.tensor(y, device=DEV), torch.tensor(idx, device=DEV),
            torch.tensor(np.asarray(lens, dtype=np.int32)))


def _module_scores(model, x, y, idx):
    was = model.training
    model.eval()
    with torch.no_grad():
        ref = model.score(x, y == -1, idx)
    model.train(was)
    return ref


def _bar(ref, valid):
    return 2e-5 * max(1.0, float(ref[valid].abs().max()))


MODELS = {
    "pe_fixed": dict(pe=dict(strategy="fixed", max_indices=1300)),
    "pe_learned": dict(pe=dict(strategy="learned", max_indices=1300)),
    # odd depths: the scorer's residual ping-pong ends in the other buffer (xsum_f = ping[N % 2], x_pe = ping[0])
    "pe_fixed_n1": dict(N=1, pe=dict(strategy="fixed", max_indices=1300)),
    "pe_learned_n3": dict(N=3, pe=dict(strategy="learned", max_indices=1300)),
    "input_norm_tanh": dict(input_norm=True, act="Tanh", out_act="Tanh"),
    "ordinal3": dict(d_output=3, out_act="Sigmoid"),
    "fc_only": dict(N=0, sizes=[48, 32], act="ReLU"),
    "dk64": dict(d=128, h=2, d_ff=128),
    "dk96": dict(d=96, h=1, d_ff=192),
}


@pytest.mark.parametrize("name", sorted(MODELS))
def test_scorer_matches_module_eval_forward(name):
    """valid entries of the scorer's grid == model.eval(); model.score(...) within the bar of
    test_fused_trainer_score_matches_module_eval_forward, at validation lengths 1x, 1.5x and > 4x the training length (up to a
    slate of 1,251), eagerly and from the captured graphs, also after training steps with dropout have moved the weights"""
    from allrank_amd.engine import FusedTrainer
    kw = MODELS[name]
    F, B, L = 24, 6, 40
    model = _model(F, **kw)
    loss, args = ("ordinal", {"n": 3}) if kw.get("d_output", 1) > 1 else ("listNet", {})
    ft = FusedTrainer(model, loss, args, B, L, lr=1e-3, use_graph=True)
    xt, yt, it, _ = _ragged([40, 25, 13, 40, 31, 2], L, F, 1)
    for Lv, lens in ((40, [40, 3, 17, 0, 39]), (60, [60, 1, 44, 59]), (1251, [1251, 7, 300, 0, 180])):
        sc_ = ft.scorer(len(lens), Lv)
        x, y, idx, hl = _ragged(lens, Lv, F, Lv)
        for step in range(4):
            ft.step(xt, yt, it)                                     # training steps (dropout on) move the weights
            out = sc_.run(x, y, idx, lengths=hl if step % 2 else None).clone()
            ref = _module_scores(model, x, y, idx)
            valid = y != -1
            sc = sc_.scores
            assert float((sc - ref)[valid].abs().max()) <= _bar(ref, valid), (name, Lv, step, sc_.last_mode)
            assert not sc[~valid].any() and not out[~valid].any()   # padded slots are 0
        assert sc_.last_mode in ("capture", "replay"), sc_.last_mode


def test_scorer_matches_fp64_oracle_on_long_validation_slates():
    """a set whose longest validation slate is > 4x the training length: scores vs oracle/model_oracle.forward in fp64, with the bar
    of the fp64 model tests (2e-5 of the score scale).  136 features and a 256-wide FC layer at 48 x 48 training rows: the trainer's
    first GEMM reads 256-float padded input rows (pad_input), so the scorer's input buffer takes that layout too"""
    from allrank_amd.engine import FusedTrainer
    from allrank_amd.model import make_model
    cfg = dict(n_features=136, fc_sizes=[256], fc_activation=None, fc_input_norm=False, N=2, d_ff=256, h=4, output_activation=None)
    params = M.init_params(cfg, seed=5)
    model = make_model(dict(sizes=[256], input_norm=False, activation=None, dropout=0.0),
                       dict(N=2, d_ff=256, h=4, positional_encoding=None, dropout=0.0), dict(d_output=1, output_activation=None), 136)
    model.load_state_dict({k: torch.tensor(v) for k, v in params.items()})
    model.to(DEV)
    ft = FusedTrainer(model, "approxNDCGLoss", {}, 48, 48, lr=1e-3, use_graph=True)
    assert ft._x_pad
    lens = [230, 1, 57, 0, 199, 120]
    x, y, idx, hl = _ragged(lens, 230, 136, 3)
    sc_ = ft.scorer(len(lens), 230)
    for _ in range(3):
        sc = sc_.run(x, y, idx, lengths=hl).clone()
    p64 = {k: v.astype(np.float64) for k, v in params.items()}
    mask = (y == -1).cpu().numpy()
    so, _ = M.forward(p64, cfg, x.cpu().numpy().astype(np.float64), mask)
    err = np.abs(sc.cpu().numpy().astype(np.float64) - so)[~mask].max()
    assert err <= 2e-5 * max(1.0, float(np.abs(so[~mask]).max())), err


def test_captured_scores_equal_eager_scores_and_lru():
    """replayed graphs == eager forward bit for bit: within one bucket (different valid counts), across a bucket change, with an
    all-padded and a one-item slate; the LRU evicts the least recently used bucket"""
    from allrank_amd.engine import FusedTrainer, row_bucket
    F, Lv = 24, 300
    model = _model(F, pe=dict(strategy="fixed", max_indices=400))
    ft = FusedTrainer(model, "listNet", {}, 4, 40, lr=1e-3, use_graph=True)
    cap = ft.scorer(5, Lv, max_graphs=2)
    eag = ft.scorer(5, Lv, use_graph=False)
    batches = [[300, 150, 0, 1, 49], [300, 150, 0, 1, 59], [299, 151, 1, 0, 60],     # 500, 510, 511 valid rows: one bucket
               [300, 300, 1, 0, 99],                                                # 700 rows: another bucket
               [20, 0, 1, 5, 6], [300, 150, 0, 1, 49]]                              # 32 rows (third bucket), back to the first
    assert len({row_bucket(sum(b)) for b in batches[:3]}) == 1 and row_bucket(700) != row_bucket(500)
    for rep in range(3):
        for k, lens in enumerate(batches):
            x, y, idx, hl = _ragged(lens, Lv, F, 10 * k + 1)
            a = cap.run(x, y, idx, lengths=hl).clone()
            b = eag.run(x, y, idx, lengths=hl).clone()
            assert torch.equal(a, b), (rep, k, cap.last_mode)
    # last round: the 704-row bucket is captured (graphs: 512, 704), the 32-row one evicts 512, the return to 512 evicts 704
    assert len(cap._graphs) == 2 and cap.evictions == 2
    assert list(cap._graphs) == [row_bucket(32), row_bucket(sum(batches[-1]))]        # LRU order: least recently used first


@pytest.mark.parametrize("world", [1, 2])
def test_assemble_packed_equals_batch_then_pack(world):
    """ltrx_assemble_packed == DeviceSlates.batch (padding branch) followed by packing, bit for bit: features (alignment rows 0),
    labels, packed-row index, positions, and the cu_seqlens the scorer uploads -- per rank block"""
    from allrank_amd import _lib as LB
    from allrank_amd.data import DeviceSlates
    from allrank_amd.parallel import shard_slates
    rng = np.random.default_rng(4)
    lens = [5, 1, 33, 17, 2, 40, 9, 28, 3]
    n_items, F = sum(lens), 136
    X = rng.standard_normal((n_items, F)).astype(np.float32)
    y = rng.integers(0, 5, n_items).astype(np.float32)
    q = np.repeat(np.arange(len(lens)), lens)
    ds = DeviceSlates(X, y, q, device=DEV)
    L = 41                                                               # above the longest slate: padding branch only
    ids = torch.tensor([7, 2, 0, 5, 8, 3, 1], dtype=torch.int64)
    lib = LB.lib()
    for rank in range(world):
        a, b = shard_slates(len(ids), rank, world)
        blk = ids[a:b]
        Bb = len(blk)
        xb, yb, ib = ds.batch(blk.to(DEV), L, seed=0)
        valid = (yb != -1).reshape(-1)
        cu = torch.zeros(Bb + 1, dtype=torch.int32)
        cu[1:] = torch.cumsum(torch.tensor([lens[i] for i in blk.tolist()]), 0)
        n = int(cu[-1])
        rows = (n + 31) // 32 * 32 + 32
        x_out = torch.full((rows, 256), 7.0, device=DEV)
        x_out[:, F:] = 0
        y_out = torch.empty((Bb, L), device=DEV)
        idx_out = torch.empty(rows, dtype=torch.int32, device=DEV)
        pos_out = torch.empty(rows, dtype=torch.int64, device=DEV)
        cu_d, ids_d = cu.to(DEV), blk.to(DEV)
        LB.check(lib.ltrx_assemble_packed(LB.ptr(ds.x_items), LB.ptr(ds.y_items), LB.ptr(ds.offsets), LB.ptr(ids_d), LB.ptr(cu_d), Bb, L, F,
                                          rows, LB.ptr(x_out), 256, LB.ptr(y_out), LB.ptr(idx_out), LB.ptr(pos_out), LB.stream_of(x_out)),
                 "assemble_packed")
        pr = torch.nonzero(valid).flatten()
        assert torch.equal(x_out[:n, :F], xb.reshape(-1, F)[pr]) and not x_out[n:].any()
        assert torch.equal(y_out, yb)
        assert torch.equal(idx_out[:n].long(), pr) and (idx_out[n:] == -1).all()
        assert torch.equal(pos_out[:n], ib.reshape(-1)[pr]) and (pos_out[n:] == -1).all()
        # the padded-batch pair: gather the valid rows back out of the padded batch, scatter them into a grid
        g = torch.full((rows, F), 3.0, device=DEV)
        gi = torch.empty(rows, dtype=torch.int32, device=DEV)
        LB.check(lib.ltrx_gather_rows_cu(LB.ptr(xb), F, LB.ptr(cu_d), Bb, L, F, rows, LB.ptr(g), F, LB.ptr(gi), LB.stream_of(g)),
                 "gather_rows_cu")
        assert torch.equal(g[:n], x_out[:n, :F]) and not g[n:].any() and torch.equal(gi, idx_out)
        grid = torch.full((Bb, L, F), 5.0, device=DEV)
        LB.check(lib.ltrx_scatter_rows_cu(LB.ptr(g), F, LB.ptr(cu_d), Bb, L, F, rows, LB.ptr(grid), F, LB.stream_of(g)), "scatter_rows_cu")
        assert torch.equal(grid, xb)


def _fit(val_scorer, tmp_path, loaders, loss=None, env=None, monkeypatch=None, epochs=2):
    from allrank_amd import fit as EF, losses as E
    torch.manual_seed(3)
    model = _model(20, pe=dict(strategy="fixed", max_indices=200))
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    cfg = types.SimpleNamespace(metrics={"ndcg": [5, 10]}, val_metric="ndcg_5")
    if env is not None:
        monkeypatch.setenv("ALLRANK_AMD_VAL_SCORER", env)
    res = EF.fit(epochs=epochs, model=model, loss_func=loss or partial(E.listNet), optimizer=opt, scheduler=None, train_dl=loaders[0],
                 valid_dl=loaders[1], config=cfg, gradient_clipping_norm=None, early_stopping_patience=10, device=torch.device(DEV),
                 output_dir=str(tmp_path), tensorboard_output_path=None, val_scorer=val_scorer)
    return res, copy.deepcopy(EF.last_run)


def _host_loaders():
    from torch.utils.data import DataLoader, TensorDataset
    tr = _ragged([int(v) for v in np.random.default_rng(1).integers(5, 31, 32)], 30, 20, 1)
    va = _ragged([int(v) for v in np.random.default_rng(2).integers(1, 150, 20)] + [150], 150, 20, 2)
    return (DataLoader(TensorDataset(*[t.cpu() for t in tr[:3]]), batch_size=16, shuffle=False),
            DataLoader(TensorDataset(*[t.cpu() for t in va[:3]]), batch_size=16, shuffle=False))


def _device_loaders(tmp_path):
    import bench
    from allrank_amd import data as ED
    rng = np.random.default_rng(9)
    for role, n in (("train", 40), ("vali", 27)):
        lens = np.clip(rng.integers(1, 200 if role == "vali" else 30, n), 1, None)
        bench.write_synth_libsvm(str(tmp_path / ("%s.txt" % role)), lens, 20, 5 if role == "train" else 6)
    tr, va = ED.load_libsvm_dataset(str(tmp_path), 30, "vali", device=DEV)
    return ED.DeviceLoader(tr, 16, shuffle=True), ED.DeviceLoader(va, 16, shuffle=False)


@pytest.mark.parametrize("kind", ["host", "resident"])
def test_fit_packed_scorer_matches_module_scorer(kind, tmp_path, monkeypatch):
    """fit(val_scorer="packed") == fit(val_scorer="module") on validation slates longer than the training slates: validation loss
    within 1e-6 relative, ndcg_5 / ndcg_10 within 1e-5; the environment variable does the same; last_run names the scorer"""
    def loaders():
        return _host_loaders() if kind == "host" else _device_loaders(tmp_path)
    res_m, run_m = _fit("module", tmp_path, loaders())
    res_p, run_p = _fit("packed", tmp_path, loaders())
    res_e, run_e = _fit(None, tmp_path, loaders(), env="packed", monkeypatch=monkeypatch)
    assert run_m["val_scorer"] == "module" and run_p["val_scorer"] == "packed" and run_e["val_scorer"] == "packed"
    assert run_p["val_scorer_reason"] == ""
    for e_m, e_p, e_e in zip(run_m["epoch_log"], run_p["epoch_log"], run_e["epoch_log"]):
        assert abs(e_p["val_loss"] - e_m["val_loss"]) <= 1e-6 * max(1.0, abs(e_m["val_loss"])), (e_p, e_m)
        assert e_e["val_loss"] == e_p["val_loss"]
    for k in ("ndcg_5", "ndcg_10"):
        assert abs(float(res_p["val_metrics"][k]) - float(res_m["val_metrics"][k])) <= 1e-5, k
        assert float(res_e["val_metrics"][k]) == float(res_p["val_metrics"][k])


def test_fit_packed_scorer_falls_back_for_stochastic_neuralndcg(tmp_path):
    from allrank_amd import losses as E
    res, run = _fit("packed", tmp_path, _host_loaders(), loss=partial(E.neuralNDCG, stochastic=True), epochs=1)
    assert run["val_scorer"] == "module" and "stochastic" in run["val_scorer_reason"]
