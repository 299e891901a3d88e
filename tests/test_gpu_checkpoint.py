"""-m gpu: checkpoint and resume at epoch boundaries, bit for bit (allrank_amd.checkpoint, FusedTrainer.state_dict /
load_state_dict, fit(checkpoint_every=..., resume=...)).

The common job: 40 training slates of 3..24 items at slate length 24 in batches of 16 (steps of 16, 16 and a short 8: the short
batch has its own batch divisor and its own captured step), 24 validation slates of up to 30 items, 10 input features (no multiple
of 4: the row-padded copy of W_0 has to be refreshed after a load), FCModel([32]) -> one encoder layer (d_model 32, h 4, d_ff 64,
dropout 0.1) -> one score, 4 epochs.  Per case three runs -- S: straight; C: with checkpoint_every=1; R: 2 epochs with
checkpoint_every=1, then a fresh model / optimizer / scheduler / loaders built under OTHER torch and numpy seeds and resume= that
file -- and C == S, R == S bitwise on every tensor of the final state_dict, on the validation losses of epochs 2 and 3 and on the
returned result.  Precondition, measured in the same test: S twice gives identical bits; where it does not (a finding: no such case
is known), the bar for that case is max |R - S| <= max |S - S'| per tensor."""
import copy
import os
import random
import types
from functools import partial

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L_TRAIN, L_VAL, BS, N_TRAIN, N_VAL = 24, 30, 16, 40, 24
NOT_REPEATABLE = ()         # cases whose uninterrupted run was found not to repeat itself bit for bit (profiles/checkpoint_resume.md): none


# ---- data ------------------------------------------------------------------------------------------------------------------------
def _slates(n, L, F, seed, lo):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, L, F)).astype(np.float32)
    w = rng.standard_normal(F).astype(np.float32)
    y = np.clip(np.round((x @ w) / np.sqrt(F) + 1.5), 0, 4).astype(np.float32)
    idx = np.tile(np.arange(L, dtype=np.int64), (n, 1))
    for b in range(n):
        k = int(rng.integers(lo, L + 1))
        y[b, k:], x[b, k:], idx[b, k:] = -1, 0, -1
    return torch.tensor(x), torch.tensor(y), torch.tensor(idx)


_HOST, _RESIDENT = {}, {}


def _host_loaders(F):
    """the reference's loaders: a shuffled host DataLoader (sampler seed from torch's global generator) and the validation one"""
    from torch.utils.data import DataLoader, TensorDataset
    if F not in _HOST:
        _HOST[F] = (TensorDataset(*_slates(N_TRAIN, L_TRAIN, F, 1, 3)), TensorDataset(*_slates(N_VAL, L_VAL, F, 2, 1)))
    tr, va = _HOST[F]
    return DataLoader(tr, batch_size=BS, shuffle=True), DataLoader(va, batch_size=BS, shuffle=False)


def _device_loaders(F, root):
    """DeviceLoader(shuffle=True, sampling="device") over a resident set in which 6 stored slates are longer than the slate length:
    their items are drawn per epoch from a seed taken from numpy's global generator"""
    import bench
    from allrank_amd import data as ED
    if F not in _RESIDENT:
        rng = np.random.default_rng(9)
        d = os.path.join(root, "set%d" % F)
        os.makedirs(d, exist_ok=True)
        lens_tr = np.concatenate([rng.integers(3, L_TRAIN + 1, N_TRAIN - 6), rng.integers(L_TRAIN + 1, 41, 6)])
        lens_va = np.concatenate([rng.integers(1, L_VAL + 1, N_VAL - 1), [L_VAL]])
        bench.write_synth_libsvm(os.path.join(d, "train.txt"), rng.permutation(lens_tr), F, 5)
        bench.write_synth_libsvm(os.path.join(d, "vali.txt"), lens_va, F, 6)
        _RESIDENT[F] = ED.load_libsvm_dataset(d, L_TRAIN, "vali", device=DEV)
    tr, va = _RESIDENT[F]
    return ED.DeviceLoader(tr, BS, shuffle=True, sampling="device"), ED.DeviceLoader(va, BS, shuffle=False)


@pytest.fixture(scope="module")
def data_root(tmp_path_factory):
    return str(tmp_path_factory.mktemp("ckpt_data"))


# ---- the cases -------------------------------------------------------------------------------------------------------------------
def _model(F=10, d=32, h=4, encoder=True, dropout=0.1):
    from allrank_amd.model import make_model
    tr = dict(N=1, d_ff=64, h=h, positional_encoding=None, dropout=dropout) if encoder else None
    return make_model(dict(sizes=[d], input_norm=False, activation=None, dropout=0.0), tr, dict(d_output=1, output_activation=None), F).to(DEV)


def _step_lr(opt):
    return torch.optim.lr_scheduler.StepLR(opt, step_size=3, gamma=0.5)


def _case(n):
    """(name -> value) of case n of the module docstring's table"""
    from allrank_amd import losses as E
    c = dict(F=10, model=_model, loss=partial(E.listNet), opt=lambda ps: torch.optim.Adam(ps, lr=2e-3), sched=_step_lr, loader="host",
             fit={}, epochs=4, patience=10, clip=None, engine="fused", fcstep=False)
    if n == 1:      # moments, step count, drop_step, numpy + torch global generators, lr by the scheduler after the resume point
        c.update(loader="device")
    elif n == 2:    # the packed step, decoupled decay, clipping, the host sampler's seed
        c.update(opt=lambda ps: torch.optim.AdamW(ps, lr=2e-3, weight_decay=0.01), clip=1.0, fit=dict(compact=True))
    elif n == 3:    # the tie-shuffle generator of ListMLE, the momentum buffer
        c.update(loss=partial(E.listMLE), opt=lambda ps: torch.optim.SGD(ps, lr=1e-2, momentum=0.9, nesterov=True))
    elif n == 4:    # the slate-resident FC + ListNet step: moments and step count written by its own Adam, raw pointers into flat_p
        c.update(F=12, model=partial(_model, F=12, encoder=False), fcstep=True)
    elif n == 5:    # Gumbel noise keyed by drop_step and the site seed
        c.update(loss=partial(E.neuralNDCG, stochastic=True, n_samples=4), loader="device")
    elif n == 6:    # the autograd engine: raw torch optimizer state, the GPU's default generator (nn.Dropout)
        c.update(opt=lambda ps: torch.optim.Adam(ps, lr=2e-3, amsgrad=True), engine="autograd")
    elif n == 7:    # scheduler and early-stopping state
        c.update(sched=lambda opt: torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="max", factor=0.5, patience=0), patience=1, epochs=6,
                 loader="device")
    elif n == 8:    # head width 40: the split-bf16 attention path's weight images after a load
        c.update(model=partial(_model, d=80, h=2), loader="device")
    return c


def _run(c, out_dir, data_root, epochs=None, seeds=(42, 43, 44), model=None, **fit_kw):
    """one fit() of case ``c`` built from scratch under ``seeds`` (torch, numpy, random); returns what the assertions read"""
    from allrank_amd import fit as EF
    torch.manual_seed(seeds[0]), np.random.seed(seeds[1]), random.seed(seeds[2])
    model = c["model"]() if model is None else model
    opt = c["opt"](model.parameters())
    sched = c["sched"](opt)
    train_dl, valid_dl = _host_loaders(c["F"]) if c["loader"] == "host" else _device_loaders(c["F"], data_root)
    os.makedirs(out_dir, exist_ok=True)
    cfg = types.SimpleNamespace(metrics={"ndcg": [5]}, val_metric="ndcg_5")
    kw = dict(c["fit"])
    kw.update(fit_kw)
    res = EF.fit(epochs=c["epochs"] if epochs is None else epochs, model=model, loss_func=c["loss"], optimizer=opt, scheduler=sched,
                 train_dl=train_dl, valid_dl=valid_dl, config=cfg, gradient_clipping_norm=c["clip"], early_stopping_patience=c["patience"],
                 device=torch.device(DEV), output_dir=out_dir, tensorboard_output_path=None, **kw)
    run = copy.deepcopy(EF.last_run)
    assert run["engine"] == c["engine"] and bool(run["fcstep"]) == c["fcstep"], run
    return dict(res=res, sd={k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, run=run, lr=opt.param_groups[0]["lr"],
                val_loss={e: r["val_loss"] for e, r in zip(range(res["epochs"] - len(run["epoch_log"]) + 1, res["epochs"] + 1), run["epoch_log"])},
                model=model, opt=opt)


def _same_result(a, b):
    return (a["epochs"] == b["epochs"] and a["num_params"] == b["num_params"] and a["train_metrics"] == b["train_metrics"]
            and a["val_metrics"] == b["val_metrics"])


def _assert_is_the_same_job(got, s, s2, what):
    """``got`` == S -- bitwise where S repeats itself bitwise (asserted to be everywhere: see the module docstring), else within S's
    own spread per tensor"""
    spread = {k: float((s["sd"][k].double() - s2["sd"][k].double()).abs().max()) for k in s["sd"]}
    print("%s: S vs S' max |diff| over tensors = %g" % (what, max(spread.values())))
    assert set(got["sd"]) == set(s["sd"])
    for k, v in s["sd"].items():
        if spread[k] == 0.0:
            assert torch.equal(got["sd"][k], v), "%s: %s differs from the uninterrupted run by %g" % (
                what, k, float((got["sd"][k].double() - v.double()).abs().max()))
        else:
            assert float((got["sd"][k].double() - v.double()).abs().max()) <= spread[k], (what, k, spread[k])
    exact = max(spread.values()) == 0.0 and _same_result(s["res"], s2["res"]) and s["val_loss"] == s2["val_loss"]
    assert got["res"]["epochs"] == s["res"]["epochs"], what
    assert got["lr"] == s["lr"], (what, got["lr"], s["lr"])
    for e in got["val_loss"]:
        tol = 0.0 if exact else abs(s["val_loss"][e] - s2["val_loss"][e])
        assert abs(got["val_loss"][e] - s["val_loss"][e]) <= tol, (what, e, got["val_loss"][e], s["val_loss"][e])
    if exact:
        assert _same_result(got["res"], s["res"]), (what, got["res"], s["res"])
    return exact


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 8])
def test_checkpointed_and_resumed_runs_are_the_uninterrupted_run(n, tmp_path, data_root):
    from allrank_amd import checkpoint as CK
    c = _case(n)
    out = lambda name: str(tmp_path / name)
    s = _run(c, out("s"), data_root)
    s2 = _run(c, out("s2"), data_root)
    # feature off: no new key, no file
    assert "checkpoint" not in s["run"] and "resume" not in s["run"] and all("ckpt_s" not in e for e in s["run"]["epoch_log"])
    assert sorted(os.listdir(out("s"))) == ["model.pkl"]
    ran = s["res"]["epochs"] + 1
    assert ran == c["epochs"] or n == 7

    ck = _run(c, out("c"), data_root, checkpoint_every=1)
    assert ck["run"]["checkpoint"] == {"path": os.path.join(out("c"), "checkpoint.pt"), "every": 1, "written": ran}
    assert all("ckpt_s" in e for e in ck["run"]["epoch_log"]) and sorted(os.listdir(out("c"))) == ["checkpoint.pt", "model.pkl"]
    exact = _assert_is_the_same_job(ck, s, s2, "case %d, checkpointing on" % n)

    first = _run(c, out("r"), data_root, epochs=2, checkpoint_every=1)
    path = first["run"]["checkpoint"]["path"]
    stored = CK.load(path)
    assert stored["epoch"] == 1 and stored["engine"] == c["engine"] and stored["n_steps"] == 6
    r = _run(c, out("r"), data_root, seeds=(7, 8, 9), checkpoint_every=1, resume=path)
    assert r["run"]["resume"] == {"path": path, "epoch": 1}
    assert len(r["run"]["epoch_log"]) == ran - 2 and sorted(r["val_loss"]) == list(range(2, ran))
    assert _assert_is_the_same_job(r, s, s2, "case %d, resumed after epoch 1" % n) == exact
    assert exact or n in NOT_REPEATABLE, "case %d: the uninterrupted run does not repeat itself bit for bit (see the printed spread)" % n

    if n == 7:      # the file of a run that has ended: nothing is trained, the stored result comes back, model.pkl is written
        os.remove(os.path.join(out("r"), "model.pkl"))
        again = _run(c, out("r"), data_root, seeds=(17, 18, 19), resume="auto")
        assert again["run"]["epoch_log"] == [] and again["run"]["resume"]["epoch"] == s["res"]["epochs"]
        assert _same_result(again["res"], s["res"]) and again["lr"] == s["lr"]
        assert all(torch.equal(again["sd"][k], v) for k, v in s["sd"].items())
        assert os.path.exists(os.path.join(out("r"), "model.pkl"))
        # resume="auto" without a file starts fresh
        fresh = _run(c, out("fresh"), data_root, epochs=1, resume="auto")
        assert "resume" not in fresh["run"] and len(fresh["run"]["epoch_log"]) == 1


# ---- the engine ------------------------------------------------------------------------------------------------------------------
def _trainer(seed, init_seed, **kw):
    from allrank_amd.engine import FusedTrainer
    torch.manual_seed(init_seed)
    model = _model()
    return FusedTrainer(model, "listNet", {}, BS, L_TRAIN, lr=2e-3, seed=seed, use_graph=True, **kw), model


def test_trainer_state_dict_restores_in_place_into_a_trainer_with_captured_graphs_and_stale_images(tmp_path):
    from allrank_amd import checkpoint as CK
    x, y, idx = (t.to(DEV) for t in _slates(5 * BS, L_TRAIN, 10, 3, 3))
    xo, yo, io = (t.to(DEV) for t in _slates(3 * BS, L_TRAIN, 10, 4, 3))
    batch = lambda t3, k: tuple(t[k * BS:(k + 1) * BS] for t in t3)
    a, model_a = _trainer(11, 1)
    losses_a = []
    for k in range(5):
        losses_a.append(a.step(*batch((x, y, idx), k)).clone())
        if k == 2:
            path = CK.save(str(tmp_path / "checkpoint.pt"), {"trainer": a.state_dict()})
    sd = CK.load(path)["trainer"]                                              # through the file
    assert sd["optimizer"]["step"] == 3 and sd["drop_step"] == 3 and sd["seed"] == a._seed and sd["lr"] == 2e-3
    for name, p in model_a.named_parameters():                                 # shaped like the parameters: no padding, no q / k / v fusion
        assert sd["params"][name].shape == p.shape and sd["optimizer"]["state"][name]["exp_avg"].shape == p.shape
        assert sd["optimizer"]["state"][name]["exp_avg_sq"].shape == p.shape
    score_a = a.score(*batch((xo, yo, io), 0)).clone()

    b, model_b = _trainer(12, 2)
    for k in range(4):                 # captured steps, a captured score(), images of OTHER weights, step words that are not A's
        b.step(*batch((xo, yo, io), k % 3))
    b.score(*batch((xo, yo, io), 1))
    assert b.last_mode in ("capture", "replay") and b._seed != a._seed
    bufs = ("flat_p", "flat_g", "flat_m", "flat_v", "step_count", "drop_step")
    ptrs = {k: getattr(b, k).data_ptr() for k in bufs}
    b.load_state_dict(sd)
    assert {k: getattr(b, k).data_ptr() for k in bufs} == ptrs                  # restored in place: nothing was rebound
    views_b = {id(r.p): r.w for r in b.params}
    assert all(p.data_ptr() == views_b[id(p)].data_ptr() for p in model_b.parameters())
    losses_b = [b.step(*batch((x, y, idx), k)).clone() for k in (3, 4)]
    assert torch.equal(losses_b[0], losses_a[3]) and torch.equal(losses_b[1], losses_a[4]), (losses_a, losses_b)
    for k in ("flat_p", "flat_m", "flat_v", "step_count", "drop_step"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert int(b.step_count.item()) == 5 and int(b.drop_step.item()) == 5
    assert torch.equal(b.score(*batch((xo, yo, io), 0)), score_a)
    assert {k: getattr(b, k).data_ptr() for k in bufs} == ptrs

    # refusal: other betas -- ValueError before any buffer changes
    c, _ = _trainer(13, 3, betas=(0.9, 0.99))
    before, ptr = c.flat_p.clone(), c.flat_p.data_ptr()
    with pytest.raises(ValueError, match="betas"):
        c.load_state_dict(sd)
    assert torch.equal(c.flat_p, before) and c.flat_p.data_ptr() == ptr and int(c.step_count.item()) == 0


@pytest.fixture(scope="module")
def case1_file(tmp_path_factory, data_root):
    """case 1's checkpoint after 2 epochs"""
    out = str(tmp_path_factory.mktemp("case1"))
    first = _run(_case(1), out, data_root, epochs=2, checkpoint_every=1)
    return first["run"]["checkpoint"]["path"]


def test_a_fused_checkpoint_resumes_under_the_autograd_engine_and_the_other_way_round(case1_file, tmp_path, data_root):
    from allrank_amd import checkpoint as CK
    from allrank_amd.engine import FusedTrainer
    stored = CK.load(case1_file)
    state = stored["trainer"]
    r = _run(dict(_case(1), engine="autograd"), str(tmp_path / "a"), data_root, epochs=stored["epoch"] + 1, seeds=(3, 4, 5), resume=case1_file,
             use_fused=False)
    assert r["run"]["epoch_log"] == [] and r["res"]["epochs"] == stored["epoch"]
    for name, p in r["model"].named_parameters():
        st = r["opt"].state[p]
        assert int(st["step"]) == state["optimizer"]["step"] == stored["n_steps"]
        assert torch.equal(st["exp_avg"].cpu(), state["optimizer"]["state"][name]["exp_avg"]), name
        assert torch.equal(st["exp_avg_sq"].cpu(), state["optimizer"]["state"][name]["exp_avg_sq"]), name
        assert torch.equal(p.detach().cpu(), state["params"][name]), name
    assert r["lr"] == state["lr"]

    # the reverse: a plain-Adam run of the autograd engine, resumed by the fused one
    auto = dict(_case(1), engine="autograd")
    first = _run(auto, str(tmp_path / "b"), data_root, epochs=2, checkpoint_every=1, use_fused=False)
    path = first["run"]["checkpoint"]["path"]
    stored = CK.load(path)
    state = stored["trainer"]
    assert stored["engine"] == "autograd" and "state" in state["optimizer"] and state["optimizer"]["step"] == 6
    r = _run(_case(1), str(tmp_path / "b"), data_root, epochs=2, seeds=(3, 4, 5), resume=path)
    assert r["run"]["engine"] == "fused" and r["run"]["epoch_log"] == []
    for name, p in r["model"].named_parameters():
        assert torch.equal(p.detach().cpu(), state["params"][name]), name
    torch.manual_seed(5)
    model = _model()
    t = FusedTrainer(model, "listNet", {}, BS, L_TRAIN, lr=2e-3)
    t.load_state_dict(state)
    back = t.state_dict()
    assert back["optimizer"]["step"] == 6 and back["lr"] == state["lr"]
    for name in state["optimizer"]["state"]:
        for slot in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(back["optimizer"]["state"][name][slot], state["optimizer"]["state"][name][slot]), (name, slot)
    n = t.nflat                                                                # the segments' padding floats stay zero
    covered = torch.zeros(n, dtype=torch.bool)
    offs = {id(r.p): r.off for r in t.params}
    for p in model.parameters():
        o = offs[id(p)]
        covered[o:o + p.numel()] = True
    assert not bool(covered.all()) and all(float(buf.cpu()[~covered].abs().max()) == 0.0 for buf in (t.flat_p, t.flat_m, t.flat_v))

    # a raw torch optimizer state (amsgrad) is tied to the autograd engine
    raw = _run(_case(6), str(tmp_path / "c"), data_root, epochs=1, checkpoint_every=1)
    with pytest.raises(ValueError, match="amsgrad|raw"):
        _run(_case(1), str(tmp_path / "c"), data_root, resume=raw["run"]["checkpoint"]["path"])


@pytest.mark.parametrize("what", ["d_ff", "betas", "loss"])
def test_resume_refuses_the_file_of_another_job_before_any_buffer_changes(what, case1_file, tmp_path, data_root):
    from allrank_amd import losses as E
    from allrank_amd.model import make_model
    c = _case(1)
    torch.manual_seed(21)
    if what == "d_ff":
        model = make_model(dict(sizes=[32], input_norm=False, activation=None, dropout=0.0),
                           dict(N=1, d_ff=128, h=4, positional_encoding=None, dropout=0.1), dict(d_output=1, output_activation=None), 10).to(DEV)
        match = "feed_forward"
    else:
        model = _model()
        match = "betas" if what == "betas" else "loss.*listNet.*approxNDCGLoss"
    if what == "betas":
        c["opt"] = lambda ps: torch.optim.Adam(ps, lr=2e-3, betas=(0.9, 0.99))
    if what == "loss":
        c["loss"] = partial(E.approxNDCGLoss)
    before = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    with pytest.raises(ValueError, match=match):
        _run(c, str(tmp_path), data_root, model=model, resume=case1_file)
    # the model's parameters are views of the trainer's flat_p: the refusal left them as they were built
    assert all(torch.equal(v.detach().cpu(), before[k]) for k, v in model.state_dict().items())
    assert not os.path.exists(os.path.join(str(tmp_path), "model.pkl"))
