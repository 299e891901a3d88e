"""No GPU: the host-side surface of the opt-in wide-head attention backward (fit's ALLRANK_AMD_WIDE_BACKWARD, the checkpoint meta key,
ltrx_mha_bwd_wide's refusal of NULL operands)."""
import types

import pytest


def test_fit_reads_the_environment_switch(monkeypatch):
    from allrank_amd.fit import _attention_option
    monkeypatch.delenv("ALLRANK_AMD_WIDE_BACKWARD", raising=False)
    assert _attention_option("wide_backward", None) is False and _attention_option("wide_backward", True) is True
    monkeypatch.setenv("ALLRANK_AMD_WIDE_BACKWARD", "0")
    assert _attention_option("wide_backward", None) is False
    monkeypatch.setenv("ALLRANK_AMD_WIDE_BACKWARD", "1")
    assert _attention_option("wide_backward", None) is True and _attention_option("wide_backward", False) is False      # an explicit argument wins
    monkeypatch.setenv("ALLRANK_AMD_WIDE_BACKWARD", "yes")
    with pytest.raises(ValueError, match="ALLRANK_AMD_WIDE_BACKWARD"):
        _attention_option("wide_backward", None)


def test_meta_carries_the_flag_only_when_it_is_on():
    from allrank_amd import checkpoint as CK
    from allrank_amd.engine import FusedTrainer

    def meta(wide):
        t = types.SimpleNamespace(_params_named=[], optimizer="Adam", _hyper=lambda: {"lr": 1e-3}, loss=types.SimpleNamespace(name="listNet"),
                                  _loss_args={}, clip=None, wide_heads=False, wide_backward=wide)
        return FusedTrainer.meta(t)

    assert "wide_backward" not in meta(False) and meta(True)["wide_backward"] is True
    for saved, live in ((True, False), (False, True)):
        with pytest.raises(ValueError, match="wide_backward"):
            CK.check_compatible(meta(saved), meta(live))


def test_null_operands_are_refused_before_any_hip_call():
    from allrank_amd import _lib, build
    build.build(verbose=False)
    assert _lib.lib().ltrx_mha_bwd_wide(None, None, None, None, None, None, None, 1, 1, 1, 96, 96, 96, None, None, None, 96, 0.0, 0, None,
                                        None, None, 1, None, None) == -1
