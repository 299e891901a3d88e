"""No GPU: every row of engine.ATTENTION_ARMS -- the opt-in attention arms -- has the whole host-side surface of an option: the keyword
on FusedTrainer and fit, the environment variable fit reads, the checkpoint meta key that exists only when the option is on, and
check_compatible's refusal of a mismatch.  A row added to the table is held to all of it."""
import inspect
import types

import pytest

from allrank_amd.engine import ATTENTION_ARMS

ARMS = pytest.mark.parametrize("arm", ATTENTION_ARMS, ids=lambda a: a.option)


def test_the_table_is_the_three_arms():
    assert [(a.option, a.env, a.direction, a.arm) for a in ATTENTION_ARMS] == [
        ("wide_heads", "ALLRANK_AMD_WIDE_HEADS", "forward", "wide"),
        ("wide_backward", "ALLRANK_AMD_WIDE_BACKWARD", "backward", "wide"),
        ("narrow_heads", "ALLRANK_AMD_NARROW_HEADS", "forward", "narrow")]          # wide before narrow: the forward's precedence


@ARMS
def test_keyword_is_accepted(arm):
    from allrank_amd import _lib, inference, kernels
    from allrank_amd.engine import FusedTrainer
    from allrank_amd.fit import fit
    assert inspect.signature(FusedTrainer.__init__).parameters[arm.option].default is False
    assert inspect.signature(fit).parameters[arm.option].default is None
    if arm.direction == "forward":
        assert inspect.signature(inference.Ranker.__init__).parameters[arm.option].default is None
        assert getattr(inference, arm.option) is False
    assert callable(getattr(_lib, arm.fits)) and arm.call is getattr(kernels, arm.call.__name__) and arm.what


@ARMS
def test_environment_variable_resolves(arm, monkeypatch):
    from allrank_amd.fit import _attention_option
    monkeypatch.delenv(arm.env, raising=False)
    assert _attention_option(arm.option, None) is False and _attention_option(arm.option, True) is True
    for off in ("", "0"):
        monkeypatch.setenv(arm.env, off)
        assert _attention_option(arm.option, None) is False
    monkeypatch.setenv(arm.env, "1")
    assert _attention_option(arm.option, None) is True and _attention_option(arm.option, False) is False      # an explicit argument wins
    for bad in ("yes", "2", "true", " 1"):
        monkeypatch.setenv(arm.env, bad)
        with pytest.raises(ValueError, match=arm.env):
            _attention_option(arm.option, None)


@ARMS
def test_meta_key_only_when_on_and_mismatch_refused(arm):
    from allrank_amd import checkpoint as CK
    from allrank_amd.engine import FusedTrainer

    def meta(on):
        t = types.SimpleNamespace(_params_named=[], optimizer="Adam", _hyper=lambda: {"lr": 1e-3}, loss=types.SimpleNamespace(name="listNet"),
                                  _loss_args={}, clip=None, **{a.option: on and a is arm for a in ATTENTION_ARMS})
        return FusedTrainer.meta(t)

    assert meta(True)[arm.option] is True
    assert not any(a.option in meta(False) for a in ATTENTION_ARMS)
    assert [a.option for a in ATTENTION_ARMS if a.option in meta(True)] == [arm.option]
    CK.check_compatible(meta(False), meta(False))
    CK.check_compatible(meta(True), meta(True))
    for saved, live in ((True, False), (False, True)):
        with pytest.raises(ValueError, match=arm.option) as e:
            CK.check_compatible(meta(saved), meta(live))
        assert arm.what in str(e.value) and "stored %r, live %r" % (saved, live) in str(e.value)
