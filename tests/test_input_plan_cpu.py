"""No GPU: the input-row plan of the fused step (engine.input_row_plan) and the library entries the odd-feature path adds.

For F % 4 == 0 the plan must be the rule the engine had before feature counts outside the multiples of 4 were taken -- written out
below as ``parent_rule`` -- because that rule decides the launch sequence of every job that ran before.  For F % 4 != 0 it must give
rows the GEMM entries accept (ltrx_gemm_nt: K and both row strides multiples of 4)."""
import ctypes
import itertools

import pytest

GEMMS = ("split_bf16", "split_bf16_strict", "hipblaslt", "bf16")
# both sides of every threshold of the rule: M >= 2048, H % 256 == 0, (F <= 1024 and F % 256 != 0 are covered by the F range)
MS = (64, 2047, 2048, 61440)
HS = (32, 96, 255, 256, 260, 512)


def parent_rule(F, H, M, gemm, has_input_norm, pad_input):
    """FusedTrainer._x_pad and the shapes _alloc_forward gave it, as they stood: dense rows, or rows of 256 floats with K = F rounded
    up to the GEMM's 32-column step"""
    x_pad = bool(pad_input and not has_input_norm and gemm in ("split_bf16", "bf16") and F % 4 == 0 and F % 256 != 0
                 and F <= 1024 and H % 256 == 0 and M >= 2048)
    if x_pad:
        return (F + 255) // 256 * 256, (F + 31) // 32 * 32, True
    return F, F, False


def test_multiples_of_four_keep_the_rule_they_had():
    from allrank_amd.engine import input_row_plan
    n_large = 0
    for F in range(4, 1025, 4):
        for H, M, gemm, norm, pad in itertools.product(HS, MS, GEMMS, (False, True), (True, False)):
            got = input_row_plan(F, H, M, gemm, norm, pad)
            assert tuple(got) == parent_rule(F, H, M, gemm, norm, pad), (F, H, M, gemm, norm, pad, got)
            n_large += bool(got[2])
    assert n_large > 0                                         # (the large-tile side of the condition was visited)


def test_other_feature_counts_get_rows_the_gemms_accept():
    from allrank_amd.engine import input_row_plan
    seen = set()
    for F in [f for f in range(1, 1030) if f % 4]:
        for H, M, gemm, norm, pad in itertools.product(HS, MS, GEMMS, (False, True), (True, False)):
            stride, K, large = input_row_plan(F, H, M, gemm, norm, pad)
            what = (F, H, M, gemm, norm, pad, stride, K, large)
            assert stride % 4 == 0 and stride >= F, what
            assert K % 4 == 0 and K >= F, what
            assert K <= stride, what
            # the 256-float form exactly where the large-tile condition holds apart from F % 4
            want_large = bool(pad and not norm and gemm in ("split_bf16", "bf16") and F <= 1024 and H % 256 == 0 and M >= 2048)
            assert large == want_large, what
            if large:
                assert stride % 256 == 0 and stride - F < 256 and K % 32 == 0 and K - F < 32, what
            else:
                assert stride == K == (F + 3) // 4 * 4, what   # no wider than the GEMM contract asks
            seen.add(large)
    assert seen == {False, True}


@pytest.fixture(scope="module")
def lib():
    from allrank_amd import build, _lib
    build.build(verbose=False)
    return _lib.lib()


def test_new_entries_are_in_the_header_and_bound(lib):
    from allrank_amd import _lib
    with open(_lib.HEADER_PATH) as fh:
        header = fh.read()
    assert "ltrx_layernorm_torch_fwd_strided(" in header and "ltrx_mha_head_width_supported(" in header
    assert _lib.PROTOTYPES["ltrx_layernorm_torch_fwd_strided"] == ("int", ["*", "int", "*", "*", "int", "int", "float", "*", "int", "*", "*",
                                                                          "ltrx_stream_t"])
    assert _lib.PROTOTYPES["ltrx_mha_head_width_supported"] == ("int", ["int"])
    assert callable(lib.ltrx_layernorm_torch_fwd_strided) and callable(lib.ltrx_mha_head_width_supported)
    # the entry it stands next to is unchanged
    assert _lib.PROTOTYPES["ltrx_layernorm_torch_fwd"] == ("int", ["*", "*", "*", "int", "int", "float", "*", "*", "*", "ltrx_stream_t"])


def test_refusals_happen_on_the_host(lib):
    p = ctypes.c_void_p(0x10000)

    def ln(x=p, ldx=48, w=p, b=p, rows=8, D=46, y=p, ldy=48, mean=p, rstd=p):
        return lib.ltrx_layernorm_torch_fwd_strided(x, ldx, w, b, rows, D, 1e-5, y, ldy, mean, rstd, None)

    for kw in (dict(x=None), dict(w=None), dict(b=None), dict(y=None), dict(mean=None), dict(rstd=None), dict(rows=0), dict(D=0),
               dict(ldx=45), dict(ldy=45), dict(ldx=0), dict(ldy=-48)):
        assert ln(**kw) == -1, kw

    assert [lib.ltrx_mha_head_width_supported(dk) for dk in (4, 8, 12, 64, 128)] == [1] * 5
    assert [lib.ltrx_mha_head_width_supported(dk) for dk in (0, -4, 1, 6, 10, 130, 132)] == [0] * 7


def test_flat_offsets_stay_16_byte_aligned_with_odd_input_norm_vectors(lib):
    """FusedTrainer._layout_parameters on the host: the two F-vectors of input_norm (F = 45, 46, 137; they head the flat buffer) must
    not shift what follows them off a 16-byte boundary -- the image refresh and the GEMMs read every segment in 16-byte pieces."""
    from allrank_amd import _lib as LB
    from allrank_amd.engine import FusedTrainer
    from allrank_amd.model import make_model
    for F in (2, 3, 45, 46, 137):
        model = make_model(dict(sizes=[32], input_norm=True, activation=None, dropout=0.0),
                           dict(N=1, d_ff=64, h=4, positional_encoding=None, dropout=0.0),
                           dict(d_output=1, output_activation=None), F)
        t = FusedTrainer.__new__(FusedTrainer)
        t.LB, t.lib, t.group, t.world, t.model = LB, lib, None, 1, model
        t._read_model(model, True, 0)
        offs = t._layout_parameters(True)
        assert t.params[0].p is model.input_layer.input_norm.weight and t.params[0].p.numel() == F
        assert all(o % 4 == 0 for o in offs) and t.nflat % 4 == 0, (F, offs)
        assert all(r.w.data_ptr() % 16 == 0 for r in t.params) and all(r.g.data_ptr() % 16 == 0 for r in t.params), F
        assert [tuple(v.shape) for v in model.state_dict().values()][:3] == [(F,), (F,), (32, F)]
