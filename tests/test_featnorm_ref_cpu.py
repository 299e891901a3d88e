"""tests/featnorm_ref.py -- the fp64 restatement the GPU tests compare the feature-normalisation kernels with -- held against the
reference script's own output (tests/golden/normalize_golden.npz, made by tests/golden/make_golden_normalize.py), and the host half of
allrank_amd/normalize.py (settings, flags, ``transform_host``, the state round trip) held against the restatement.  No GPU.

Bars: an entry of a column with std > 0 equals the script's after the cast to fp32, bit for bit; every entry stays within the derived
tolerance ulp32(want) + n 2^-53 (|t| + |mean|) / (std + eps), n = training items.  The script's output for a constant column is its
own cancellation noise over eps, which the tolerance covers."""
import json
import os

import numpy as np
import pytest

from oracle.ref_loader import reference_available
from tests import featnorm_ref as R


def _settings(name):
    if name == "b":                                      # the script ran with no list arguments: its defaults are the settings file
        with open(R.SETTINGS_WEB30K) as fh:
            s = json.load(fh)
        return s["features_without_logarithm"], s["features_negative"], s["eps_log"], s["eps"]
    return tuple(R.golden_case(name)["lists"]) + (1e-2, 1e-6)


@pytest.mark.parametrize("name", ["a", "b"])
def test_the_restatement_reproduces_the_reference_script(name):
    case = R.golden_case(name)
    without, negative, eps_log, eps = _settings(name)
    fit = R.fit(case["roles"], without, negative, eps_log, eps)
    assert fit["no_log_negative"] == case["no_log_negative"]
    flat = fit["std"] == 0
    assert flat.tolist() == ([f in (2, 3) for f in range(12)] if name == "a" else [False] * 136)
    for role in R.ROLES:
        want, got = case["ref"][role], fit["out"][role]
        assert want.shape == got.shape and np.isfinite(got).all()
        assert np.array_equal(got[:, ~flat].astype(np.float32), want[:, ~flat].astype(np.float32)), (name, role)
        ratio = np.abs(got - want) / R.tolerance(want, fit["t"][role], fit["mean"], fit["std"], fit["n"], eps)
        assert ratio.max() <= 1.0, (name, role, ratio.max())


def test_case_a_covers_what_it_documents():
    case = R.golden_case("a")
    x = case["roles"]
    assert [len(np.unique(case["qid"][r])) for r in R.ROLES] == [20, 7, 6]
    assert all(1 <= c <= 8 for r in R.ROLES for c in np.unique(case["qid"][r], return_counts=True)[1])
    every = np.concatenate([x[r] for r in R.ROLES])
    assert (every[:, 2] == 3).all() and (every[:, 3] == 0).all() and (every[:, 6] <= 0).all() and (every[:, 11] != 0).all()
    assert every[:, 7].min() < 0 < every[:, 7].max()
    assert x["train"][:, 8].min() >= 0 and x["test"][:, 8].min() >= 0 and x["vali"][:, 8].min() < 0
    assert x["train"][:, 10].min() >= 0 and x["vali"][:, 10].min() >= 0 and x["test"][:, 10].min() < 0
    assert every.max() == 2.0 ** 20 and every[every > 0].min() == 2.0 ** -10
    # without test.txt exactly the documented column changes its decision
    negate, want = R.flags(12, *case["lists"])
    three, _ = R.decide(want, [R.column_min(x[r], negate) for r in R.ROLES])
    two, _ = R.decide(want, [R.column_min(x[r], negate) for r in ("train", "vali")])
    assert np.flatnonzero(three != two).tolist() == np.load(R.GOLDEN)["a.only_test_decides"].tolist() == [10]


@pytest.mark.skipif(not reference_available(), reason="needs a checkout of allegro/allRank (ALLRANK_REFERENCE)")
def test_committed_fixtures_equal_a_fresh_run_of_the_maker():
    from tests.golden import make_golden_normalize as M
    built = M.build()
    with open(R.SETTINGS_WEB30K) as fh:
        assert json.load(fh) == built["normalize_web30k.json"]
    committed, fresh = np.load(R.GOLDEN), built["normalize_golden.npz"]
    assert set(committed.files) == set(fresh)
    for k in committed.files:
        a, b = committed[k], np.asarray(fresh[k])
        assert a.shape == b.shape and a.dtype == b.dtype, k
        if k.endswith(".normalized"):                     # the script's fp64 arithmetic: numpy's sums may differ between builds
            assert np.allclose(a, b, rtol=1e-12, atol=1e-7), k
        else:
            assert np.array_equal(a, b), k


# ---- the host half of allrank_amd.normalize ------------------------------------------------------------------------------
def test_settings_file_and_flags(tmp_path):
    from allrank_amd.normalize import FeatureNormalizer
    nz = FeatureNormalizer.from_settings(R.SETTINGS_WEB30K)
    with open(R.SETTINGS_WEB30K) as fh:
        s = json.load(fh)
    assert (list(nz.features_without_logarithm), list(nz.features_negative), nz.eps_log, nz.eps) == \
        (s["features_without_logarithm"], s["features_negative"], 1e-2, 1e-6)
    negate, want = nz.flags(46)                          # indices >= F are ignored
    rn, rw = R.flags(46, s["features_without_logarithm"], s["features_negative"])
    assert np.array_equal(negate, rn) and np.array_equal(want, rw) and negate.sum() == 0 and want.sum() == 46 - sum(i < 46 for i in s["features_without_logarithm"])
    assert FeatureNormalizer().flags(3)[1].tolist() == [1, 1, 1]
    bad = tmp_path / "bad.json"
    bad.write_text(json.dumps({"features_negative": [1], "surprise": 2}))
    with pytest.raises(ValueError, match="surprise"):
        FeatureNormalizer.from_settings(str(bad))
    with pytest.raises(OSError):
        FeatureNormalizer.from_settings(str(tmp_path / "absent.json"))


@pytest.mark.parametrize("name", ["a", "b"])
def test_transform_host_and_the_state_round_trip(name, tmp_path):
    from allrank_amd.normalize import FeatureNormalizer
    case = R.golden_case(name)
    without, negative, eps_log, eps = _settings(name)
    fit = R.fit(case["roles"], without, negative, eps_log, eps)
    nz = FeatureNormalizer(without, negative, eps_log, eps)
    with pytest.raises(RuntimeError, match="fit"):
        nz.transform_host(case["roles"]["train"])
    nz.load_state_dict(dict(FeatureNormalizer(without, negative, eps_log, eps).settings(), negate=fit["negate"], take_log=fit["take_log"],
                            mean=fit["mean"], std=fit["std"], roles=["train", "test", "vali"], no_log_negative=fit["no_log_negative"]))
    path = str(tmp_path / "feature_normalization.npz")
    nz.save(path)
    back = FeatureNormalizer.load(path)
    assert back.report == {"roles": ["train", "test", "vali"], "log": int(fit["take_log"].sum()), "no_log_negative": fit["no_log_negative"]}
    state = back.state_dict()
    assert state["mean"].dtype == np.float64 and state["std"].dtype == np.float64
    assert np.array_equal(state["mean"], fit["mean"]) and np.array_equal(state["take_log"], fit["take_log"])
    for role in R.ROLES:
        got = back.transform_host(case["roles"][role])
        assert got.dtype == np.float64 and np.array_equal(got, fit["out"][role])
    with pytest.raises(ValueError, match="features"):
        back.transform_host(np.zeros((2, 5), dtype=np.float32))
