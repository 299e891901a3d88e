"""-m gpu: feature normalisation on the device -- the three kernels of allrank_amd/csrc/ltrx_featnorm.hip against the fp64 restatement
(tests/featnorm_ref.py), ``FeatureNormalizer`` against the reference script's own output (tests/golden/normalize_golden.npz), the
switch behind ``load_libsvm_dataset`` against the script's ``_normalized`` files, and what ``fit`` records.  Every comparison is with
the restatement or the golden, never with the code under test.

Bars.  ``min_out``: equal.  mean and std: within n 2^-53 relative of the restatement (n rows), the std of a constant column within
sqrt(n) 2^-53 |mean| absolute.  Normalised values: within ulp32(want) + n 2^-53 (|t| + |mean|) / (std + eps).  Goldens: a column with
std > 0 equals the script's output after the cast to fp32, every entry is within that tolerance.  Each test prints its worst figure
as a fraction of its bar before it asserts.

For n = 1 the mean bar is half an ulp, i.e. the device's fp64 logarithm must equal the correctly rounded one.  It is not correctly
rounded everywhere: on 3219 probed arguments (0 .. 199, 2^-10 .. 2^20, 3000 random eighths, each + 1e-2) it differed from the exact
value, and from numpy's, on 2, by one ulp.  The committed n = 1 inputs meet the bar as it stands; measured worst figures of the other
cases: mean <= 0.07, std <= 0.30, normalised values 0.50 of their bars."""
import copy
import functools
import json
import logging
import os
import types
from functools import partial

import numpy as np
import pytest
import torch

from tests import featnorm_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS_LOG, EPS = 1e-2, 1e-6
GUARD = 64                                                # elements behind every output, bytes behind the workspace
NS, FS = (1, 63, 64, 65, 257, 4097), (1, 3, 12, 46, 136, 137)
WIDE = (45, 700, 1100)                                    # odd; more than 256 columns (4-byte form) and more than 1024 (16-byte form):
#                                                           a row then takes more than one column tile of 256 threads


@functools.lru_cache(maxsize=None)
def _reference(n, F):
    """the contract case of (n, F) and its restatement, made once and shared (never written to)"""
    negate, take_log = R.contract_flags(F, shift=n + F)
    x = R.contract_input(n, F, negate, take_log, seed=10000 * F + n)
    t = R.transform(x, negate, take_log, EPS_LOG)
    mean, std = R.moments(t)
    ref = dict(x=x, negate=negate, take_log=take_log, t=t, mean=mean, std=std, min=R.column_min(x, negate),
               out=R.standardize(t, mean, std, EPS), constant=(x == x[:1]).all(axis=0))
    for v in ref.values():
        v.setflags(write=False)
    return ref


def test_contract_inputs_hold_what_they_promise():
    seen = set()
    for n, F in [(n, F) for n in NS for F in FS] + [(65, F) for F in WIDE]:
        ref = _reference(n, F)
        combos = set(zip(ref["negate"].tolist(), ref["take_log"].tolist()))
        assert len(combos) == min(F, 4)
        seen |= combos
        s_x = R.signed(ref["x"], ref["negate"])
        assert (s_x[:, ref["take_log"].astype(bool)] >= 0).all() and ref["constant"][0]
        if F >= 3:
            assert (ref["x"] == 0).all(axis=0).any()
        if F >= 12:                                                             # (any four neighbours hold a column without logarithm)
            assert (s_x[n - 1] < 0).any()
        if F >= 12 and n >= 63:
            zero = np.flatnonzero((ref["x"] == 0).all(axis=0))[0]
            assert len(set(np.signbit(ref["x"][:, zero]))) == 2                  # zeros of both signs
            last = np.flatnonzero(s_x[n - 1] < 0)
            assert any((s_x[:n - 1, c] >= 0).all() for c in last)               # a column negative in its last row only
    assert len(seen) == 4


class _Guarded(object):
    """a device buffer of ``count`` elements with GUARD sentinel elements behind it"""

    def __init__(self, count, dtype, sentinel):
        self.full = torch.full((count + GUARD,), sentinel, dtype=dtype, device=DEV)
        self.t, self.count, self.sentinel = self.full[:count], count, sentinel

    def intact(self):
        return bool((self.full[self.count:] == self.sentinel).all())


def _run_kernels(ref, n, F, ld):
    """one pass of the three kernels over a fresh copy of the case, rows ``ld`` floats apart, the gaps and the tail filled with NaN"""
    from allrank_amd import _lib as LB, normalize as N
    lib = LB.lib()
    buf = torch.full((n * ld + GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    x = buf[:n * ld].view(n, ld)[:, :F]
    x.copy_(torch.from_numpy(ref["x"].copy()))
    before = buf.clone()
    negate, take_log = (torch.from_numpy(ref[k].copy()).to(DEV) for k in ("negate", "take_log"))
    mn, mean, std = _Guarded(F, torch.float32, -7.0), _Guarded(F, torch.float64, -7.0), _Guarded(F, torch.float64, -7.0)
    ws_min = _Guarded(lib.ltrx_feature_min_workspace_bytes(n, F), torch.uint8, 0xA5)
    ws_mom = _Guarded(lib.ltrx_feature_moments_workspace_bytes(n, F), torch.uint8, 0xA5)
    st = LB.stream_of(x)
    N.feature_min(lib, st, x, n, negate, mn.t, ws_min.t)
    N.feature_moments(lib, st, x, n, negate, take_log, EPS_LOG, mean.t, std.t, ws_mom.t)
    torch.cuda.synchronize()
    assert torch.equal(buf.view(torch.int32), before.view(torch.int32)), "a reduction wrote to its input"
    N.feature_normalize(lib, st, x, n, negate, take_log, EPS_LOG, mean.t, std.t, EPS)
    torch.cuda.synchronize()
    outside = torch.ones(n * ld + GUARD, dtype=torch.bool, device=DEV)
    outside[:n * ld].view(n, ld)[:, :F] = False
    assert torch.equal(buf.view(torch.int32)[outside], before.view(torch.int32)[outside]), "the gap behind a row or the tail was written"
    assert all(g.intact() for g in (mn, mean, std, ws_min, ws_mom)), "a guard behind an output or a workspace was written"
    return mn.t.cpu().numpy(), mean.t.cpu().numpy(), std.t.cpu().numpy(), x.cpu().numpy()


@pytest.mark.parametrize("pad", [0, 3], ids=["ld=F", "ld=F+3"])
@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("n", NS)
def test_kernel_contract(n, F, pad):
    _contract(n, F, pad)


@pytest.mark.parametrize("pad", [0, 3], ids=["ld=F", "ld=F+3"])
@pytest.mark.parametrize("F", WIDE)
def test_kernel_contract_wide_rows(F, pad):
    _contract(65, F, pad)


def _contract(n, F, pad):
    ref = _reference(n, F)
    got_min, got_mean, got_std, got_x = _run_kernels(ref, n, F, F + pad)
    u = 2.0 ** -53
    mean_bar = n * u * np.abs(ref["mean"])
    std_bar = np.where(ref["constant"], np.sqrt(n) * u * np.abs(ref["mean"]), n * u * np.abs(ref["std"]))
    tol = R.tolerance(ref["out"], ref["t"], ref["mean"], ref["std"], n, EPS)
    mean_err, std_err, out_err = np.abs(got_mean - ref["mean"]), np.abs(got_std - ref["std"]), np.abs(got_x.astype(np.float64) - ref["out"])

    def worst(err, bar):
        return float(np.max(np.where(err == 0, 0.0, err / np.where(bar > 0, bar, np.finfo(np.float64).tiny))))
    print("n %d F %d ld %d: mean %.3g  std %.3g  normalised %.3g of the bar" % (n, F, F + pad, worst(mean_err, mean_bar),
                                                                               worst(std_err, std_bar), worst(out_err, tol)))
    assert np.array_equal(got_min, ref["min"])
    assert np.isfinite(got_x).all()
    assert (mean_err <= mean_bar).all(), ("mean", np.flatnonzero(mean_err > mean_bar)[:8], worst(mean_err, mean_bar))
    assert (std_err <= std_bar).all(), ("std", np.flatnonzero(std_err > std_bar)[:8], worst(std_err, std_bar))
    assert (out_err <= tol).all(), ("normalised", worst(out_err, tol))
    again = _run_kernels(ref, n, F, F + pad)
    for a, b in zip((got_min, got_mean, got_std, got_x), again):
        assert a.tobytes() == b.tobytes(), "a repeated call gave other bits"


# ---- FeatureNormalizer against the reference script ---------------------------------------------------------------------------
def _settings(name):
    if name == "b":
        with open(R.SETTINGS_WEB30K) as fh:
            return json.load(fh)
    without, negative = R.golden_case(name)["lists"]
    return dict(features_without_logarithm=without, features_negative=negative, eps_log=EPS_LOG, eps=EPS)


def _slates(case, role):
    from allrank_amd.data import DeviceSlates
    return DeviceSlates(case["roles"][role], case["y"][role], case["qid"][role], device=DEV)


def _check_against_script(name, case, fitted, got, label):
    """``got`` {role: f32 array} against the script's output at the CPU test's bars"""
    flat = fitted["std"] == 0
    for role, have in got.items():
        want = case["ref"][role]
        tol = R.tolerance(want, fitted["t"][role], fitted["mean"], fitted["std"], fitted["n"], EPS)
        err = np.abs(have.astype(np.float64) - want)
        print("%s case %s %s: worst %.3g of the tolerance" % (label, name, role, float((err / tol).max())))
        assert have.dtype == np.float32 and np.array_equal(have[:, ~flat], want[:, ~flat].astype(np.float32)), (label, name, role)
        assert (err <= tol).all(), (label, name, role, float((err / tol).max()))


@pytest.mark.parametrize("name", ["a", "b"])
def test_normalizer_reproduces_the_reference_script(name):
    from allrank_amd.normalize import FeatureNormalizer
    case, s = R.golden_case(name), _settings(name)
    fitted = R.fit(case["roles"], s["features_without_logarithm"], s["features_negative"], s["eps_log"], s["eps"])
    slates = {r: _slates(case, r) for r in R.ROLES}
    nz = FeatureNormalizer(**s).fit(slates["train"], others=(slates["test"], slates["vali"]), roles=R.ROLES)
    assert nz.report == {"roles": list(R.ROLES), "log": int(fitted["take_log"].sum()), "no_log_negative": case["no_log_negative"]}
    assert np.array_equal(nz.take_log, fitted["take_log"]) and np.array_equal(nz.negate, fitted["negate"])
    for r in R.ROLES:
        nz.apply(slates[r])
    with pytest.raises(RuntimeError, match="already"):
        nz.apply(slates["train"])
    _check_against_script(name, case, fitted, {r: slates[r].x_items.cpu().numpy() for r in R.ROLES}, "FeatureNormalizer")
    # the saved state reproduces the device values on the host
    host = FeatureNormalizer().load_state_dict(nz.state_dict())
    _check_against_script(name, case, fitted, {r: host.transform_host(case["roles"][r]).astype(np.float32) for r in R.ROLES}, "transform_host")


# ---- behind load_libsvm_dataset ------------------------------------------------------------------------------------------------
def _write_roles(path, case, arrays, fmt, roles=R.ROLES):
    os.makedirs(path, exist_ok=True)
    for r in roles:
        R.write_libsvm(os.path.join(path, r + ".txt"), arrays[r], case["y"][r], case["qid"][r], fmt)


def _settings_file(tmp_path, name="a"):
    path = str(tmp_path / "settings.json")
    with open(path, "w") as fh:
        json.dump(_settings(name), fh)
    return path


def test_load_libsvm_dataset_normalizes_like_the_script(tmp_path, monkeypatch, caplog):
    from allrank_amd import data as ED
    case = R.golden_case("a")
    raw, done = str(tmp_path / "ds"), str(tmp_path / "ds_normalized")
    _write_roles(raw, case, case["roles"], "%.17g")
    _write_roles(done, case, case["ref"], "%.16g")           # the script's files: dump_svmlight_file prints %.16g
    monkeypatch.delenv(ED.NORMALIZE_ENV, raising=False)
    plain = ED.load_libsvm_dataset(raw, 6, "vali", device=DEV)
    theirs = ED.load_libsvm_dataset(done, 6, "vali", device=DEV)
    assert not hasattr(plain[0], "normalizer")
    # unset: the device parse of the raw files, bit for bit what it always was -- the fixture's fp32 values
    for ds, role in zip(plain, ("train", "vali")):
        assert ds.slates.x_items.cpu().numpy().tobytes() == case["roles"][role].tobytes()
    monkeypatch.setenv(ED.NORMALIZE_ENV, _settings_file(tmp_path))
    with caplog.at_level(logging.INFO, logger="allrank_amd.data"):
        ours = ED.load_libsvm_dataset(raw, 6, "vali", device=DEV)
    assert ours[0].normalizer is ours[1].normalizer and ours[0].normalizer.roles == ["train", "test", "vali"]
    assert ours[0].normalizer.report["no_log_negative"] == case["no_log_negative"]
    assert "for the sign decision only" in caplog.text and "test.txt" in caplog.text
    fitted = R.fit(case["roles"], *case["lists"])
    for a, b, role in zip(ours, theirs, ("train", "vali")):
        assert a.slate_length == b.slate_length
        for k in ("y_items", "offsets", "lengths"):
            assert torch.equal(getattr(a.slates, k), getattr(b.slates, k)), (role, k)
        got, want = a.slates.x_items.cpu().numpy().astype(np.float64), b.slates.x_items.cpu().numpy().astype(np.float64)
        tol = R.tolerance(want, fitted["t"][role], fitted["mean"], fitted["std"], fitted["n"], EPS)
        print("end to end %s: worst %.3g of the tolerance" % (role, float((np.abs(got - want) / tol).max())))
        assert (np.abs(got - want) <= tol).all(), role
    # the keyword is the same switch
    monkeypatch.delenv(ED.NORMALIZE_ENV)
    keyword = ED.load_libsvm_dataset(raw, 6, "vali", device=DEV, normalize=_settings_file(tmp_path))
    assert all(torch.equal(k.slates.x_items, o.slates.x_items) for k, o in zip(keyword, ours))
    monkeypatch.setenv(ED.NORMALIZE_ENV, str(tmp_path / "absent.json"))
    with pytest.raises(OSError, match=ED.NORMALIZE_ENV):
        ED.load_libsvm_dataset(raw, 6, "vali", device=DEV)


def test_a_missing_role_is_logged_and_changes_only_the_documented_columns(tmp_path, caplog):
    from allrank_amd import data as ED
    case = R.golden_case("a")
    raw = str(tmp_path / "ds")
    _write_roles(raw, case, case["roles"], "%.17g", roles=("train", "vali"))
    with caplog.at_level(logging.INFO, logger="allrank_amd.data"):
        train, _ = ED.load_libsvm_dataset(raw, 6, "vali", device=DEV, normalize=_settings_file(tmp_path))
    nz = train.normalizer
    assert nz.roles == ["train", "vali"] and nz.report["roles"] == ["train", "vali"]
    assert "test.txt is missing" in caplog.text
    full = R.fit(case["roles"], *case["lists"])
    assert np.flatnonzero(nz.take_log != full["take_log"]).tolist() == np.load(R.GOLDEN)["a.only_test_decides"].tolist()
    two = R.fit({r: case["roles"][r] for r in ("train", "vali")}, *case["lists"])
    assert np.array_equal(nz.take_log, two["take_log"]) and nz.no_log_negative == two["no_log_negative"]


# ---- fit ---------------------------------------------------------------------------------------------------------------------------
def _fit_one_epoch(tmp_path, loaders):
    """one epoch of the small job of tests/test_gpu_packed_scorer.py (its model helper; case "a" has 12 features)"""
    from allrank_amd import fit as EF, losses as E
    from tests.test_gpu_packed_scorer import _model
    torch.manual_seed(3)
    model = _model(12, pe=dict(strategy="fixed", max_indices=200))
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    cfg = types.SimpleNamespace(metrics={"ndcg": [5, 10]}, val_metric="ndcg_5")
    EF.fit(epochs=1, model=model, loss_func=partial(E.listNet), optimizer=opt, scheduler=None, train_dl=loaders[0], valid_dl=loaders[1],
           config=cfg, gradient_clipping_norm=None, early_stopping_patience=10, device=torch.device(DEV), output_dir=str(tmp_path),
           tensorboard_output_path=None)
    return copy.deepcopy(EF.last_run)


def test_fit_writes_the_normalization_beside_the_model(tmp_path):
    from allrank_amd import data as ED, fit as EF
    from allrank_amd.normalize import FeatureNormalizer
    case = R.golden_case("a")
    raw = str(tmp_path / "ds")
    _write_roles(raw, case, case["roles"], "%.17g")
    fitted = R.fit(case["roles"], *case["lists"])
    out = {}
    for switch in (True, False):
        tr, va = ED.load_libsvm_dataset(raw, 6, "vali", device=DEV, normalize=_settings_file(tmp_path) if switch else None)
        out[switch] = tmp_path / ("run_%s" % switch)
        out[switch].mkdir()
        run = _fit_one_epoch(out[switch], (ED.DeviceLoader(tr, 8, shuffle=True), ED.DeviceLoader(va, 8, shuffle=False)))
        assert (out[switch] / "model.pkl").exists()
        if not switch:
            assert "normalize" not in run and not (out[switch] / EF.NORMALIZATION_FILE).exists()
            continue
        assert run["normalize"] == {"roles": ["train", "test", "vali"], "log": int(fitted["take_log"].sum()),
                                    "no_log_negative": case["no_log_negative"]}
        back = FeatureNormalizer.load(str(out[switch] / EF.NORMALIZATION_FILE))
        for ds, role in ((tr, "train"), (va, "vali")):
            want = back.transform_host(case["roles"][role])
            got = ds.slates.x_items.cpu().numpy().astype(np.float64)
            tol = R.tolerance(want, fitted["t"][role], fitted["mean"], fitted["std"], fitted["n"], EPS)
            assert (np.abs(got - want) <= tol).all(), role
