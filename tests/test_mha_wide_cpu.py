"""No GPU: the host-side surface of the opt-in wide-head attention forward (ltrx_mha_wide_fits, fit's ALLRANK_AMD_WIDE_HEADS,
the checkpoint meta key)."""
import types

import pytest


def test_wide_fits_truth_table():
    from allrank_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.lib()
    for dk in (60, 64, 68, 72, 96, 128, 130, 132):
        for L in (0, 1, 289):
            want = int(L > 0 and 64 < dk <= 128 and dk % 4 == 0)
            assert lib.ltrx_mha_wide_fits(L, dk) == want, (L, dk)
    assert lib.ltrx_mha_wide_fits(128 * 65535, 96) == 1 and lib.ltrx_mha_wide_fits(128 * 65535 + 1, 96) == 0      # the grid limit
    # refused before any HIP call: a mode the kernel does not have, a NULL operand
    assert lib.ltrx_mha_fwd_wide(None, None, None, None, 1, 1, 1, 96, 96, None, 96, None, 0.0, 0, None, None, None, 1, None) == -1


def test_fit_reads_the_environment_switch(monkeypatch):
    from allrank_amd.fit import _attention_option
    monkeypatch.delenv("ALLRANK_AMD_WIDE_HEADS", raising=False)
    assert _attention_option("wide_heads", None) is False and _attention_option("wide_heads", True) is True
    monkeypatch.setenv("ALLRANK_AMD_WIDE_HEADS", "0")
    assert _attention_option("wide_heads", None) is False
    monkeypatch.setenv("ALLRANK_AMD_WIDE_HEADS", "1")
    assert _attention_option("wide_heads", None) is True and _attention_option("wide_heads", False) is False      # an explicit argument wins
    monkeypatch.setenv("ALLRANK_AMD_WIDE_HEADS", "yes")
    with pytest.raises(ValueError, match="ALLRANK_AMD_WIDE_HEADS"):
        _attention_option("wide_heads", None)


def test_meta_carries_the_flag_only_when_it_is_on():
    from allrank_amd import checkpoint as CK
    from allrank_amd.engine import FusedTrainer

    def meta(wide):
        t = types.SimpleNamespace(_params_named=[], optimizer="Adam", _hyper=lambda: {"lr": 1e-3}, loss=types.SimpleNamespace(name="listNet"),
                                  _loss_args={}, clip=None, wide_heads=wide)
        return FusedTrainer.meta(t)

    assert "wide_heads" not in meta(False) and meta(True)["wide_heads"] is True
    CK.check_compatible(meta(False), meta(False))
    CK.check_compatible(meta(True), meta(True))
    for saved, live in ((True, False), (False, True)):
        with pytest.raises(ValueError, match="wide_heads"):
            CK.check_compatible(meta(saved), meta(live))
