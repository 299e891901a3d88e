"""No GPU: install(inference=True) puts allrank_amd.inference.rank_slates behind the reference's second entry point, the golden ranking
fixture has not drifted from the live reference, and the module path of our rank_slates (what a model on the CPU takes) returns the
reference's result.  The reference-dependent tests need the reference tree, as tests/test_install_cpu.py does."""
import importlib
import inspect

import numpy as np
import pytest
import torch

from oracle.ref_loader import reference_available
from tests import rank_cases as RC

needs_reference = pytest.mark.skipif(not reference_available(), reason="reference tree only exists in the build container")


def _reference_modules():
    from oracle.ref_loader import load_reference
    load_reference()
    ru = importlib.import_module("allrank.inference.inference_utils")
    rc = importlib.import_module("allrank.rank_and_click")
    return ru, rc


@needs_reference
def test_install_inference_rebinds_both_names_and_uninstall_restores():
    import allrank_amd
    from allrank_amd import inference as EI
    ru, rc = _reference_modules()
    ref = ru.rank_slates
    assert rc.rank_slates is ref
    done = allrank_amd.install(inference=True, data=False)
    try:
        assert ru.rank_slates is EI.rank_slates and rc.rank_slates is EI.rank_slates
        assert {"allrank.inference.inference_utils.rank_slates", "allrank.rank_and_click.rank_slates"} <= set(done)
        assert inspect.signature(EI.rank_slates) == inspect.signature(ref)
    finally:
        allrank_amd.uninstall()
    assert ru.rank_slates is ref and rc.rank_slates is ref


@needs_reference
def test_plain_install_leaves_the_inference_names_untouched():
    import allrank_amd
    ru, rc = _reference_modules()
    ref = ru.rank_slates
    plain = allrank_amd.install(data=False)
    try:
        assert ru.rank_slates is ref and rc.rank_slates is ref
        assert not [n for n in plain if "rank_slates" in n]
        # the default call's list: exactly what install(inference=True) returns without its two names
        allrank_amd.uninstall()
        with_inf = allrank_amd.install(data=False, inference=True)
        assert [n for n in with_inf if "rank_slates" not in n] == plain
    finally:
        allrank_amd.uninstall()
    assert "inference" in inspect.signature(allrank_amd.install).parameters
    assert inspect.signature(allrank_amd.install).parameters["inference"].default is False


@needs_reference
def test_signature_equals_the_references():
    from allrank_amd import inference as EI
    ru, _ = _reference_modules()
    ours, ref = inspect.signature(EI.rank_slates), inspect.signature(ru.rank_slates)
    # names, kinds and defaults always; the annotations (the reference's own classes) once install(inference=True) has bound it
    assert [(p.name, p.kind, p.default) for p in ours.parameters.values()] == [(p.name, p.kind, p.default) for p in ref.parameters.values()]


@needs_reference
def test_committed_rank_golden_equals_the_live_reference():
    """the drift guard of tests/test_golden_drift.py for make_golden_rank (that test lists its generators by name)"""
    state = torch.get_rng_state()
    try:
        built = importlib.import_module("tests.golden.make_golden_rank").build()
    finally:
        torch.set_rng_state(state)
    assert list(built) == ["rank_golden.npz"]
    committed, fresh = RC.golden(), built["rank_golden.npz"]
    assert set(committed) == set(fresh), sorted(set(committed) ^ set(fresh))
    for k in committed:
        a, b = np.asarray(committed[k]), np.asarray(fresh[k])
        assert a.shape == b.shape and a.dtype.kind == b.dtype.kind, (k, a.shape, b.shape, a.dtype, b.dtype)
        if a.dtype.kind in "iub":
            assert np.array_equal(a, b), k
        elif a.dtype.kind in "US":
            assert (a == b).all(), k
        elif k in ("ranked_x", "ranked_y", "x", "y"):                 # copies of the inputs: exact
            assert np.array_equal(a, b), k
        else:
            assert np.isfinite(a).all() and np.isfinite(b).all(), k
            err = np.abs(a.astype(np.float64) - b.astype(np.float64)) / (1.0 + np.abs(a.astype(np.float64)))
            assert float(err.max()) <= 1e-6, (k, float(err.max()))


def test_golden_fixture_states_its_gap_and_dtypes():
    """the committed scores keep the generator's gap condition: adjacent scores of a slate at least 1e-3 * max(1, max|s|) apart"""
    g = RC.golden()
    assert str(g["dtype_x"]) == "torch.float32" and str(g["dtype_y"]) == "torch.float32"
    assert g["ranked_x"].shape == g["x"].shape and g["ranked_y"].shape == g["y"].shape
    for b, k in enumerate(g["lens"]):
        s = g["scores"][b, :k]
        if k > 1:
            assert np.diff(np.sort(s)).min() >= float(g["min_gap"]) * max(1.0, float(np.abs(s).max())), b
        # and the stored ranking is the descending order of those scores
        o = np.argsort(-s, kind="stable")
        assert np.array_equal(g["ranked_y"][b, :k], g["y"][b, :k][o]) and (g["ranked_y"][b, k:] == -1).all()
        assert np.array_equal(g["ranked_x"][b, :k], g["x"][b, :k][o]) and not g["ranked_x"][b, k:].any()


@needs_reference
def test_module_path_on_cpu_returns_the_golden_ranking_with_a_reason():
    """CPU tensors (the reference's own model, on the host): never an exception -- the nn.Module path, which equals the reference's
    stored result exactly.  (An allrank_amd model has no CPU forward: its layers are the HIP kernels.)"""
    from allrank_amd import inference as EI
    _reference_modules()
    from allrank.models.model import make_model
    from allrank.config import TransformerConfig, PositionalEncoding
    g = RC.golden()
    tr = TransformerConfig(N=int(g["cfg.N"]), d_ff=int(g["cfg.d_ff"]), h=int(g["cfg.h"]), dropout=0.0,
                           positional_encoding=PositionalEncoding(strategy="fixed", max_indices=int(g["cfg.max_indices"])))
    model = make_model(dict(sizes=[int(v) for v in g["cfg.fc_sizes"]], input_norm=False, activation=None, dropout=0.0), tr,
                       dict(d_output=1, output_activation=None), int(g["cfg.n_features"]))
    model.load_state_dict({k.split(".", 1)[1]: torch.tensor(v) for k, v in g.items() if k.startswith(("param.", "buffer."))})
    out = EI.rank_slates({"test": RC.HostSlates(g["x"], g["y"])}, model, RC.config(int(g["cfg.batch_size"])))
    X, y = out["test"]
    assert EI.last_run["engine"] == "module" and "CPU" in EI.last_run["reason"]
    assert str(X.dtype) == str(g["dtype_x"]) and str(y.dtype) == str(g["dtype_y"]) and not X.is_cuda
    assert np.array_equal(X.numpy().view(np.uint32), g["ranked_x"].view(np.uint32))
    assert np.array_equal(y.numpy(), g["ranked_y"])


def test_rank_slates_cu_states_the_call_by_header_name():
    """the launcher's one ltrx_* call against the header's parameter names, both source forms (the form of
    tests/test_kernel_calls_cpu.py, whose recorder and expectation helper it borrows)"""
    import types
    from tests.test_kernel_calls_cpu import Recorder, _expect, ST, f32, i32, i64
    from allrank_amd import inference as EI
    B, L, F, ml = 3, 7, 12, 5
    scores, cu, order, perm = f32(11), i32(B + 1), i32(B), i32(11)
    x, y, x_out, y_out = f32(B, L, F), f32(B, L), f32(B, L, F), f32(B, L)
    rec = Recorder()
    EI.rank_slates_cu(rec, ST, scores, cu, order, B, ml, L, x_out, y_out, perm, x=x, y=y)
    _expect(rec, "ltrx_rank_slates_cu", scores=scores.data_ptr(), x=x.data_ptr(), y=y.data_ptr(), x_items=None, y_items=None,
            offsets=None, ids=None, cu_seqlens=cu.data_ptr(), slate_order=order.data_ptr(), B=B, max_len=ml, F=F, L=L,
            perm=perm.data_ptr(), x_out=x_out.data_ptr(), y_out=y_out.data_ptr(), stream=ST.value)
    slates = types.SimpleNamespace(x_items=f32(40, F), y_items=f32(40), offsets=i64(9))
    ids = i64(B)
    rec = Recorder()
    EI.rank_slates_cu(rec, ST, scores, cu, None, B, ml, L, x_out, y_out, slates=slates, ids=ids)
    _expect(rec, "ltrx_rank_slates_cu", scores=scores.data_ptr(), x=None, y=None, x_items=slates.x_items.data_ptr(),
            y_items=slates.y_items.data_ptr(), offsets=slates.offsets.data_ptr(), ids=ids.data_ptr(), cu_seqlens=cu.data_ptr(),
            slate_order=None, B=B, max_len=ml, F=F, L=L, perm=None, x_out=x_out.data_ptr(), y_out=y_out.data_ptr(), stream=ST.value)
