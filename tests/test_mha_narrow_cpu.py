"""No GPU: the host-side surface of the opt-in narrow-head attention forward (ltrx_mha_narrow_fits, fit's ALLRANK_AMD_NARROW_HEADS,
the checkpoint meta key)."""
import types

import pytest


def test_narrow_fits_truth_table():
    from allrank_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.lib()
    for dk in (0, 4, 20, 30, 32, 36, 64):
        for L in (0, 1, 289):
            want = int(L > 0 and 0 < dk <= 32 and dk % 4 == 0)
            assert lib.ltrx_mha_narrow_fits(L, dk) == want == int(_lib.mha_narrow_fits(L, dk)), (L, dk)
    assert lib.ltrx_mha_narrow_fits(128 * 65535, 32) == 1 and lib.ltrx_mha_narrow_fits(128 * 65535 + 1, 32) == 0      # the grid limit
    # refused before any HIP call: a NULL operand
    assert lib.ltrx_mha_fwd_narrow(None, None, None, None, 1, 1, 1, 32, 32, None, 32, None, 0.0, 0, None, None, None, 1, None) == -1


def test_fit_reads_the_environment_switch(monkeypatch):
    from allrank_amd.fit import _attention_option
    monkeypatch.delenv("ALLRANK_AMD_NARROW_HEADS", raising=False)
    assert _attention_option("narrow_heads", None) is False and _attention_option("narrow_heads", True) is True
    monkeypatch.setenv("ALLRANK_AMD_NARROW_HEADS", "0")
    assert _attention_option("narrow_heads", None) is False
    monkeypatch.setenv("ALLRANK_AMD_NARROW_HEADS", "1")
    assert _attention_option("narrow_heads", None) is True and _attention_option("narrow_heads", False) is False      # an explicit argument wins
    monkeypatch.setenv("ALLRANK_AMD_NARROW_HEADS", "yes")
    with pytest.raises(ValueError, match="ALLRANK_AMD_NARROW_HEADS"):
        _attention_option("narrow_heads", None)


def test_meta_carries_the_flag_only_when_it_is_on():
    from allrank_amd import checkpoint as CK
    from allrank_amd.engine import FusedTrainer

    def meta(narrow):
        t = types.SimpleNamespace(_params_named=[], optimizer="Adam", _hyper=lambda: {"lr": 1e-3}, loss=types.SimpleNamespace(name="listNet"),
                                  _loss_args={}, clip=None, wide_heads=False, narrow_heads=narrow)
        return FusedTrainer.meta(t)

    assert "narrow_heads" not in meta(False) and meta(True)["narrow_heads"] is True
    CK.check_compatible(meta(False), meta(False))
    CK.check_compatible(meta(True), meta(True))
    for saved, live in ((True, False), (False, True)):
        with pytest.raises(ValueError, match="narrow_heads"):
            CK.check_compatible(meta(saved), meta(live))
