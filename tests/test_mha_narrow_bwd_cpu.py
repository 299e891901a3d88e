"""No GPU: the host side of the opt-in narrow-head attention backward (ltrx_mha_bwd_narrow's declaration, "both", the checkpoint meta)."""
import types

import pytest


def test_the_entry_is_declared_bound_and_refuses_null_operands():
    from allrank_amd import _lib, build
    build.build(verbose=False)
    assert _lib.PROTOTYPES["ltrx_mha_bwd_narrow"] == _lib.PROTOTYPES["ltrx_mha_bwd_wide"]
    assert _lib.lib().ltrx_mha_bwd_narrow(None, None, None, None, None, None, None, 1, 1, 1, 32, 32, 32, None, None, None, 32, 0.0, 0, None,
                                          None, None, 1, None, None) == -1


def test_both_is_a_value_of_narrow_heads_alone(monkeypatch):
    from allrank_amd.fit import _attention_option
    monkeypatch.setenv("ALLRANK_AMD_NARROW_HEADS", "both")
    assert _attention_option("narrow_heads", None) == "both" and _attention_option("narrow_heads", True) is True
    monkeypatch.delenv("ALLRANK_AMD_NARROW_HEADS")
    assert _attention_option("narrow_heads", "both") == "both"
    for option, env in (("wide_heads", "ALLRANK_AMD_WIDE_HEADS"), ("wide_backward", "ALLRANK_AMD_WIDE_BACKWARD")):
        with pytest.raises(ValueError, match=option):
            _attention_option(option, "both")
        monkeypatch.setenv(env, "both")
        with pytest.raises(ValueError, match=env):
            _attention_option(option, None)


def test_meta_tells_both_from_true():
    from allrank_amd import checkpoint as CK
    from allrank_amd.engine import FusedTrainer

    def meta(narrow):
        return FusedTrainer.meta(types.SimpleNamespace(_params_named=[], optimizer="Adam", _hyper=lambda: {"lr": 1e-3}, _loss_args={}, clip=None,
                                                       loss=types.SimpleNamespace(name="listNet"), wide_heads=False, narrow_heads=narrow))

    assert meta("both")["narrow_heads"] == "both"
    CK.check_compatible(meta("both"), meta("both"))
    for saved, live in ((True, "both"), ("both", True), ("both", False)):
        with pytest.raises(ValueError, match="narrow_heads"):
            CK.check_compatible(meta(saved), meta(live))
