"""allrank_amd.checkpoint without a GPU: the file (atomic write, weights_only read, refusals), the generator states, the neutral
optimizer schema on torch.optim.Adam / AdamW / SGD, ``check_compatible``, the option / environment parsing, fit()'s signature."""
import copy
import inspect
import os
import random

import numpy as np
import pytest
import torch

from allrank_amd import checkpoint as CK


def _equal(a, b):
    if torch.is_tensor(a) or torch.is_tensor(b):
        return torch.is_tensor(a) and torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_equal(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_equal(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and a == b


def _state():
    return {"epoch": 3, "lr": 1e-3, "name": "listNet", "flag": True, "nothing": None, "betas": (0.9, 0.999), "sizes": [1, 2, 3],
            "inf": float("inf"), "big": 0xFFFFFFFF, "nested": {"w": torch.arange(7, dtype=torch.float32).reshape(7, 1), 0: {"step": torch.tensor(3.0)}},
            "bytes": torch.arange(16, dtype=torch.uint8), "i64": torch.tensor([2 ** 40, -1])}


def test_save_load_round_trip_of_every_value_type(tmp_path):
    path = str(tmp_path / "checkpoint.pt")
    st = _state()
    assert CK.save(path, st) == path
    got = CK.load(path)
    assert got.pop("format") == CK.FORMAT and got.pop("magic") == CK.MAGIC
    assert _equal(got, st), (got, st)
    raw = torch.load(path, map_location="cpu", weights_only=True)              # no code runs when the file is read
    assert raw["format"] == CK.FORMAT
    assert os.listdir(str(tmp_path)) == ["checkpoint.pt"]                      # no .tmp left behind
    # what is not plain is converted on the way in: numpy scalars and arrays, ordered mappings
    import collections
    CK.save(path, {"m": np.float32(0.25), "n": np.int64(7), "a": np.arange(3, dtype=np.int32), "o": collections.OrderedDict(x=1)})
    got = CK.load(path)
    assert got["m"] == 0.25 and type(got["m"]) is float and got["n"] == 7 and type(got["n"]) is int and type(got["o"]) is dict
    assert torch.equal(got["a"], torch.tensor([0, 1, 2], dtype=torch.int32))
    assert "epoch" not in got                                                  # the second save replaced the first
    assert os.listdir(str(tmp_path)) == ["checkpoint.pt"]
    with pytest.raises(TypeError, match="state\\['f'\\]"):
        CK.save(path, {"f": lambda: 0})
    assert os.listdir(str(tmp_path)) == ["checkpoint.pt"] and "m" in CK.load(path)     # a refused save leaves the old file whole


def test_truncated_foreign_and_other_format_files_raise_naming_the_path(tmp_path):
    path = str(tmp_path / "checkpoint.pt")
    CK.save(path, _state())
    blob = open(path, "rb").read()
    cut = str(tmp_path / "cut.pt")
    with open(cut, "wb") as f:
        f.write(blob[:len(blob) // 2])
    with pytest.raises(ValueError, match="cut.pt"):
        CK.load(cut)
    text = str(tmp_path / "notes.pt")
    with open(text, "w") as f:
        f.write("not a checkpoint\n")
    with pytest.raises(ValueError, match="notes.pt"):
        CK.load(text)
    other = str(tmp_path / "model.pkl")                                        # a torch file, but not one of ours
    torch.save({"w": torch.zeros(2)}, other)
    with pytest.raises(ValueError, match="model.pkl.*not an allrank_amd checkpoint"):
        CK.load(other)
    bumped = str(tmp_path / "bumped.pt")
    body = torch.load(path, weights_only=True)
    body["format"] = CK.FORMAT + 1
    torch.save(body, bumped)
    with pytest.raises(ValueError, match="bumped.pt.*format %d" % (CK.FORMAT + 1)):
        CK.load(bumped)
    with pytest.raises(FileNotFoundError):
        CK.load(str(tmp_path / "absent.pt"))


def test_capture_and_restore_rng_repeat_the_draws(tmp_path):
    torch.manual_seed(11), np.random.seed(12), random.seed(13)
    np.random.standard_normal(3)                                               # (leaves a cached gaussian behind: part of the state)
    random.gauss(0, 1)
    path = str(tmp_path / "checkpoint.pt")
    CK.save(path, {"rng": CK.capture_rng("cpu")})

    def draws():
        return (torch.rand(5), torch.randperm(9), np.random.randint(0, 2 ** 31 - 1), np.random.standard_normal(3), np.random.permutation(6),
                random.random(), random.gauss(0, 1), random.getrandbits(70))
    first = draws()
    torch.manual_seed(99), np.random.seed(98), random.seed(97)
    CK.restore_rng(CK.load(path)["rng"], "cpu")                                # through the file: tensors and ints only
    again = draws()
    for a, b in zip(first, again):
        assert (torch.equal(a, b) if torch.is_tensor(a) else np.array_equal(a, b)), (a, b)
    assert CK.capture_rng(None)["cuda"] is None


class _Three(torch.nn.Module):
    """three parameters: one element, 15 elements (no multiple of 4), 8 elements"""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(5)
        self.scale = torch.nn.Parameter(torch.randn(1, generator=g))
        self.w = torch.nn.Parameter(torch.randn(3, 5, generator=g))
        self.b = torch.nn.Parameter(torch.randn(8, generator=g))

    def loss(self, k):
        x = torch.arange(1, 6, dtype=torch.float32) * (k + 1) / 7.0
        return ((self.w @ x).sum() * self.scale).pow(2).sum() + (self.b * (k + 2)).sin().sum()


_OPTS = {"Adam": lambda ps: torch.optim.Adam(ps, lr=1e-2, betas=(0.8, 0.95), eps=1e-7, weight_decay=0.01),
         "AdamW": lambda ps: torch.optim.AdamW(ps, lr=1e-2, weight_decay=0.05),
         "SGD": lambda ps: torch.optim.SGD(ps, lr=1e-2, momentum=0.9, nesterov=True, weight_decay=0.01)}


def _steps(model, opt, ks):
    for k in ks:
        opt.zero_grad()
        model.loss(k).backward()
        opt.step()


@pytest.mark.parametrize("kind", ["Adam", "AdamW", "SGD"])
@pytest.mark.parametrize("n_steps", [0, 3])
def test_neutral_optimizer_state_round_trip(kind, n_steps, tmp_path):
    model = _Three()
    opt = _OPTS[kind](model.parameters())
    _steps(model, opt, range(n_steps))
    neutral = CK.to_neutral(opt, model.named_parameters())
    assert neutral["kind"] == kind and set(neutral["state"]) == {"scale", "w", "b"}
    assert neutral["step"] == (0 if kind == "SGD" else n_steps)                # (torch's SGD keeps no step count)
    assert set(neutral["hyper"]) == {"lr", "betas", "eps", "weight_decay", "momentum", "nesterov"}
    for name, p in model.named_parameters():
        for slot, t in neutral["state"][name].items():
            assert t.shape == p.shape and t.device.type == "cpu", (name, slot)      # shaped like the parameter, unpadded
            src = opt.state.get(p, {}).get(slot)
            assert torch.equal(t, src if src is not None else torch.zeros_like(p)), (name, slot)
    path = str(tmp_path / "checkpoint.pt")
    CK.save(path, {"optimizer": neutral, "params": {n: p for n, p in model.named_parameters()}})
    ck = CK.load(path)
    # a fresh model and optimizer, parameters in place, state from the file
    model2 = _Three()
    with torch.no_grad():
        for n, p in model2.named_parameters():
            p.copy_(ck["params"][n])
    opt2 = _OPTS[kind](model2.parameters())
    _steps(model2, opt2, [5])                                                  # (state that the load has to replace, not add to)
    with torch.no_grad():
        for n, p in model2.named_parameters():
            p.copy_(ck["params"][n])
    CK.from_neutral(opt2, model2.named_parameters(), ck["optimizer"])
    assert _equal(CK.to_neutral(opt2, model2.named_parameters()), neutral)     # bitwise
    _steps(model, opt, [n_steps])
    _steps(model2, opt2, [n_steps])
    for (n, p), (_, q) in zip(model.named_parameters(), model2.named_parameters()):
        assert torch.equal(p, q), n
    assert _equal(CK.to_neutral(opt2, model2.named_parameters()), CK.to_neutral(opt, model.named_parameters()))


def test_neutral_refuses_differing_steps_and_keeps_other_optimizers_raw():
    model = _Three()
    opt = _OPTS["Adam"](model.parameters())
    _steps(model, opt, range(2))
    opt.state[model.w]["step"] = opt.state[model.w]["step"] + 1
    with pytest.raises(ValueError, match="step counts differ"):
        CK.to_neutral(opt, model.named_parameters())
    # a class (or an option) the schema does not cover: its own state_dict, resumable by the same class only
    model = _Three()
    ams = torch.optim.Adam(model.parameters(), lr=1e-2, amsgrad=True)
    _steps(model, ams, range(2))
    raw = CK.to_neutral(ams, model.named_parameters())
    assert raw["kind"] == "Adam" and "state" not in raw and raw["hyper"]["amsgrad"] is True
    assert set(raw["torch_optimizer"]) == {"state", "param_groups"}
    model2 = copy.deepcopy(model)
    ams2 = torch.optim.Adam(model2.parameters(), lr=5e-3, amsgrad=True)
    CK.from_neutral(ams2, model2.named_parameters(), raw)
    assert ams2.param_groups[0]["lr"] == 5e-3                                  # the rate is the caller's to restore
    _steps(model, ams, [2])
    _steps(model2, ams2, [2])
    ams2.param_groups[0]["lr"] = 1e-2
    assert all(torch.equal(ams.state[p]["max_exp_avg_sq"], ams2.state[q]["max_exp_avg_sq"]) for p, q in zip(model.parameters(), model2.parameters()))
    with pytest.raises(ValueError, match="raw Adam"):
        CK.from_neutral(torch.optim.RMSprop(model2.parameters()), model2.named_parameters(), raw)
    with pytest.raises(ValueError, match="optimizer kind"):
        CK.from_neutral(_OPTS["SGD"](model2.parameters()), model2.named_parameters(), CK.to_neutral(_OPTS["Adam"](model.parameters()), model.named_parameters()))


def _meta(**kw):
    named = kw.pop("named", [("a.weight", torch.zeros(3, 5)), ("a.bias", torch.zeros(3))])
    a = dict(kind="Adam", hyper=CK.hyper("Adam", 1e-3, (0.9, 0.999), 1e-8, 0.0), loss="neuralNDCG", args={"temperature": 1.0, "k": None}, clip=1.0)
    a.update(kw)
    return CK.make_meta(named, a["kind"], a["hyper"], a["loss"], a["args"], a["clip"])


def test_check_compatible_names_the_first_difference(tmp_path):
    path = str(tmp_path / "checkpoint.pt")
    CK.save(path, {"meta": _meta()})
    saved = CK.load(path)["meta"]                                              # as a resume sees it: through the file
    CK.check_compatible(saved, _meta())
    CK.check_compatible(saved, _meta(hyper=CK.hyper("Adam", 5e-4, (0.9, 0.999), 1e-8, 0.0)))          # lr is state, not configuration
    for live, named in ((_meta(named=[("a.weight", torch.zeros(3, 5)), ("a.b", torch.zeros(3))]), "a.b"),
                        (_meta(named=[("a.weight", torch.zeros(3, 6)), ("a.bias", torch.zeros(3))]), r"a.weight.*\(3, 5\).*\(3, 6\)"),
                        (_meta(kind="AdamW"), "optimizer kind.*Adam.*AdamW"),
                        (_meta(hyper=CK.hyper("Adam", 1e-3, (0.9, 0.99), 1e-8, 0.0)), "betas"),
                        (_meta(hyper=CK.hyper("Adam", 1e-3, (0.9, 0.999), 1e-8, 0.01)), "weight_decay"),
                        (_meta(loss="listNet"), "loss.*neuralNDCG.*listNet"),
                        (_meta(args={"temperature": 0.5, "k": None}), "temperature"),
                        (_meta(args={"temperature": 1.0, "k": None, "stochastic": True}), "stochastic"),
                        (_meta(clip=2.0), "gradient_clipping_norm"),
                        (_meta(clip=None), "gradient_clipping_norm")):
        with pytest.raises(ValueError, match=named):
            CK.check_compatible(saved, live)


def test_options_from_arguments_and_environment():
    assert CK.options(None, None, {}) == (None, None)
    assert CK.options(2, "auto", {}) == (2, "auto")
    assert CK.options(None, None, {CK.ENV_EVERY: "5", CK.ENV_RESUME: "AUTO"}) == (5, "auto")
    assert CK.options(None, None, {CK.ENV_EVERY: "", CK.ENV_RESUME: ""}) == (None, None)
    assert CK.options(None, None, {CK.ENV_RESUME: "/runs/a/checkpoint.pt"}) == (None, "/runs/a/checkpoint.pt")
    assert CK.options(3, "x.pt", {CK.ENV_EVERY: "5", CK.ENV_RESUME: "auto"}) == (3, "x.pt")          # arguments win
    for bad in ("0", "-2", "1.5", "often", "2 epochs"):
        with pytest.raises(ValueError, match=CK.ENV_EVERY):
            CK.options(None, None, {CK.ENV_EVERY: bad})
    with pytest.raises(ValueError, match=CK.ENV_RESUME):
        CK.options(None, None, {CK.ENV_RESUME: "  "})
    for bad in (0, -1, 1.5, True, "2"):
        with pytest.raises(ValueError, match="checkpoint_every"):
            CK.options(bad, None, {})
    for bad in ("", 3, True):
        with pytest.raises(ValueError, match="resume"):
            CK.options(None, bad, {})


def test_options_read_the_process_environment(monkeypatch):
    monkeypatch.setenv(CK.ENV_EVERY, "4")
    monkeypatch.delenv(CK.ENV_RESUME, raising=False)
    assert CK.options() == (4, None)
    monkeypatch.setenv(CK.ENV_EVERY, "none")
    with pytest.raises(ValueError):
        CK.options()


def test_fit_keeps_the_reference_signature_and_appends_the_two_options():
    from allrank_amd import fit as EF
    names = list(inspect.signature(EF.fit).parameters)
    assert names[:13] == ["epochs", "model", "loss_func", "optimizer", "scheduler", "train_dl", "valid_dl", "config", "gradient_clipping_norm",
                          "early_stopping_patience", "device", "output_dir", "tensorboard_output_path"]          # train_utils.py:78-79
    assert names[-3:] == ["val_scorer", "checkpoint_every", "resume"]
    assert all(inspect.signature(EF.fit).parameters[n].default is None for n in names[-2:])
