"""-m gpu: the package makes the libltrx calls, and computes the bits, it did before the GEMM, attention, LayerNorm and head calls of
allrank_amd/ops.py and allrank_amd/engine.py moved into the launchers of allrank_amd/kernels.py.

tests/golden/call_trace_parent.json was recorded by tests/golden/make_call_trace_fixture.py at the parent of that change (the commit
named in the file): per case the trace of every library call -- name, integers and floats as passed, pointers as NULL or not -- and
SHA-256 digests of losses, gradients, parameters and scores that two runs at that commit agreed on bit for bit.  Every case is run
again here through the same code and must give the same trace and the same digests.  ``gemm="hipblaslt"`` has no digests (torch's
GEMMs choose their own algorithm): its trace alone is held.

tests/golden/call_trace_rows_parent.json is the generator's second case set (``--set rows``), recorded the same way at the parent of
the change that gave the three row layouts one staging path (allrank_amd/rows.py) and the packing calls their launchers: the
cu_seqlens layout of the trainer and of the scorer, with host lengths and counted on the device, and the index layout's positions.
It is held under the same rules.

tests/golden/call_trace_step_parent.json is the third set (``--set step``), recorded at the parent of the change that moved the
training step's own calls, the ranking call and the click call into allrank_amd/kernels.py: what the two sets above do not reach --
the slate-resident FC + ListNet step in its three forms, SGD with Nesterov momentum and without a momentum buffer,
``first_nonfinite`` (its return value digested too), ``inference.rank_batches`` from a padded batch and from a resident set, and
``clicks.click_on_slates`` with a cascade and a diverse plan.  The same rules again.

tests/golden/call_trace_options_parent.json is the fourth set (``--set options``), recorded at the parent of the change that made the
step's operands records built once at construction: each A/B switch of the large-tile step off on its own, the two-group
weight-gradient composition under sublayer dropout, a three-layer FC stack, the fixed positional encoding on the padded grid,
``score()`` between two steps, ``load_state_dict`` with another seed, and a scorer over an ``input_norm`` model with 46 features.
Its traces begin at the constructor, so the size and support queries made there are held as well.  The same rules once more.

tests/golden/call_trace_fit_parent.json is the fifth set (``--set fit``), recorded at the parent of the change that gave the two
engines one interface under ``fit()``, ``_evaluate`` one score source per batch and the epoch statistics one accumulator: whole
``fit()`` calls over a small libsvm set the generator writes (40 queries of 3 to 20 items, batches of 16, so the last one is
short) -- both engines, the four validation score sources, the ragged evaluation, schedulers, early stopping, the finiteness
check with its full error text, checkpoint and resume.  A case holds the trace of the whole call and digests of the returned dict
(every value as ``float.hex`` with its type name), of ``last_run`` without wall-clock entries and paths, of the per-epoch
validation loss, of every tensor of ``model.pkl`` and, where one is written, of the checkpoint; its ``notes`` -- the engine, how
many batches each score source served, the error text -- are held like the digests.  The file stores each distinct call once and
a trace as indices into that table (``expand``)."""
import json

import pytest

from tests.golden import make_call_trace_fixture as G

pytestmark = pytest.mark.gpu


def _load(path):
    with open(path) as fh:
        return G.expand(json.load(fh))


@pytest.fixture(scope="module")
def rec():
    return _load(G.FIXTURE)


@pytest.fixture(scope="module")
def recs():
    return {name: _load(path) for name, (path, _) in G.SETS.items()}


@pytest.fixture(scope="module")
def proxy():
    with G.proxied() as p:
        yield p


def test_fixture_is_the_parents_and_covers_every_case(rec):
    assert len(rec["commit"]) == 40
    assert sorted(rec["cases"]) == sorted(G.cases())
    for name, c in rec["cases"].items():
        assert c["trace"] and c["unstable"] == [], name
        assert bool(c["digests"]) == (name != "gemm_hipblaslt"), name
    trainers = [c for n, c in rec["cases"].items() if {"loss1", "loss2", "loss3", "flat_g", "flat_p", "scores"} <= set(c["digests"])]
    assert len(trainers) >= 11
    called = {call[0] for c in rec["cases"].values() for call in c["trace"]}
    assert {"ltrx_gemm_nt", "ltrx_gemm_tn", "ltrx_mha_fwd", "ltrx_mha_bwd", "ltrx_layernorm_fwd", "ltrx_layernorm_bwd",
            "ltrx_layernorm_bwd_partial", "ltrx_score_head_fwd", "ltrx_score_head_bwd", "ltrx_out_act_fwd", "ltrx_out_act_bwd",
            "ltrx_gather_rows_cu", "ltrx_gemm_tn_group_ln", "ltrx_norm_head_fwd", "ltrx_mha_bwd_workspace_bytes",
            "ltrx_gemm_tn_workspace_bytes", "ltrx_layernorm_bwd_workspace_bytes", "ltrx_score_head_bwd_workspace_bytes"} <= called
    acts = {call[1][11] for c in rec["cases"].values() for call in c["trace"] if call[0] == "ltrx_gemm_nt"}
    assert acts == {0, 1, 2, 3, 4, 5}                        # every epilogue of ltrx_gemm_nt, the one-bit mask pair included


def test_rows_fixture_is_the_parents_and_covers_every_case(recs):
    rec = recs["rows"]
    assert len(rec["commit"]) == 40
    assert sorted(rec["cases"]) == sorted(G.rows_cases()) and len(rec["cases"]) == 7
    for name, c in rec["cases"].items():
        assert c["trace"] and c["unstable"] == [] and c["digests"], name
    called = {call[0] for c in rec["cases"].values() for call in c["trace"]}
    assert {"ltrx_ingest_batch", "ltrx_gather_rows", "ltrx_scatter_rows", "ltrx_packed_row_index", "ltrx_gather_rows_cu",
            "ltrx_scatter_rows_cu", "ltrx_zero_rows_cu", "ltrx_assemble_packed", "ltrx_posenc_fwd"} <= called
    assert not set(rec["cases"]) & set(recs["calls"]["cases"])


def test_step_fixture_is_the_parents_and_covers_every_case(recs):
    rec = recs["step"]
    assert len(rec["commit"]) == 40
    assert sorted(rec["cases"]) == sorted(G.step_cases()) and len(rec["cases"]) == 10
    for name, c in rec["cases"].items():
        assert c["trace"] and c["unstable"] == [] and c["digests"], name
    called = {call[0] for c in rec["cases"].values() for call in c["trace"]}
    assert {"ltrx_fc_listnet_step", "ltrx_fc_linear_listnet_step", "ltrx_sgd_step", "ltrx_clip_grad_norm_scale", "ltrx_first_nonfinite",
            "ltrx_rank_slates_cu", "ltrx_click_slates_cu"} <= called
    sgd = {n: [call[1] for call in rec["cases"][n]["trace"] if call[0] == "ltrx_sgd_step"] for n in rec["cases"]}
    assert sgd["sgd_no_momentum"][0][2] == 0 and sgd["sgd_nesterov_weight_decay"][0][2] == 1     # the momentum buffer: NULL, and not
    assert not set(rec["cases"]) & (set(recs["calls"]["cases"]) | set(recs["rows"]["cases"]))


def test_options_fixture_is_the_parents_and_covers_every_case(recs):
    rec = recs["options"]
    assert len(rec["commit"]) == 40
    assert sorted(rec["cases"]) == sorted(G.options_cases()) and len(rec["cases"]) == 11
    for name, c in rec["cases"].items():
        assert c["trace"] and c["unstable"] == [] and c["digests"], name
        assert c["trace"][0][0] == "ltrx_mha_head_width_supported", name                  # every trace begins at the constructor
    calls = {n: [call[0] for call in c["trace"]] for n, c in rec["cases"].items()}
    # what each switch turns off is absent from its case and present in a case that leaves it on
    b_image = lambda n: {call[1][4] for call in rec["cases"][n]["trace"] if call[0] == "ltrx_gemm_nt"}  # noqa: E731
    assert b_image("large_weight_images_off") == {0} and b_image("large_group_wgrad_off") == {1}
    assert "ltrx_gemm_tn_group_ln" not in calls["large_group_wgrad_off"] and calls["large_group_wgrad_off"].count("ltrx_gemm_tn") == 5
    assert "ltrx_gemm_tn_group_ln" not in calls["large_ln_in_wgrad_off"] and "ltrx_gemm_tn_group" in calls["large_ln_in_wgrad_off"]
    assert "ltrx_norm_head_fwd" not in calls["large_norm_head_off"] and "ltrx_norm_head_fwd" in calls["large_pad_input_off"]
    first_nt = {n: next(call[1] for call in rec["cases"][n]["trace"] if call[0] == "ltrx_gemm_nt") for n in calls}
    assert first_nt["large_pad_input_off"][1] == 136 and first_nt["large_norm_head_off"][1] == 256      # row stride of the FC operand
    # both sublayer dropouts on: two grouped launches per layer, and the constructor asks about three compositions
    assert calls["large_sublayer_dropout"].count("ltrx_debug_tn_group_plan") == 2
    assert calls["large_sublayer_dropout"].count("ltrx_gemm_tn_group_workspace_bytes") == 3
    assert calls["fc_stack_three_relu_dropout"].count("ltrx_gemm_tn") == 3 and "ltrx_relu_bwd" in calls["fc_stack_three_relu_dropout"]
    assert "ltrx_posenc_fwd" in calls["fixed_pe_grid"] and "ltrx_scale_inplace" in calls["fixed_pe_grid"]
    assert calls["step_score_step"].count("ltrx_adam_step") == 2 and calls["step_score_step"].count("ltrx_score_head_fwd") == 3
    assert calls["reload_other_seed"].count("ltrx_weight_images") == 4                      # construction, two steps, the stale images
    assert calls["scorer_input_norm_46"].count("ltrx_layernorm_torch_fwd_strided") == 2
    assert not set(rec["cases"]) & (set(recs["calls"]["cases"]) | set(recs["rows"]["cases"]) | set(recs["step"]["cases"]))


def test_fit_fixture_is_the_parents_and_covers_every_case(recs):
    rec = recs["fit"]
    assert len(rec["commit"]) == 40
    assert sorted(rec["cases"]) == sorted(G.fit_cases()) and len(rec["cases"]) == 17
    for name, c in rec["cases"].items():
        assert c["trace"] and c["unstable"] == [] and c["digests"], name
    notes = {n: c["notes"] for n, c in rec["cases"].items()}
    served = lambda n: {k for k, v in notes[n]["sources"].items() if v}  # noqa: E731
    assert {"resident", "packed", "trainer_score", "module"} == set().union(*(served(n) for n in notes))     # the four score sources
    assert served("fit_fused_grid_trainer_score") == {"trainer_score"} and served("fit_fused_grid_module_val") == {"module"}
    assert served("fit_fused_compact_graph_packed_val") == {"resident"} and served("fit_fused_host_loader_ragged_val") == {"packed"}
    assert {v["engine"] for v in notes.values()} == {"fused", "autograd"}
    assert notes["fit_fused_host_loader_ragged_val"]["val_eval"] == {"loss": "ragged", "metrics": "ragged"}       # both ragged evaluations
    assert notes["fit_fc_listnet_step"]["fcstep"] and not notes["fit_fc_listnet_step"]["compact"]
    assert notes["fit_fused_compact_graph_packed_val"]["compact_graph"] and notes["fit_fused_compact"]["compact"]
    assert "stochastic NeuralNDCG" in notes["fit_stochastic_neural_ndcg_packed_val"]["val_scorer_reason"]
    assert notes["fit_fused_step_lr_early_stop"]["epochs"] < 7                                 # early stopping fired
    assert "gradient element(s)" in notes["fit_check_finite_nan_fused"]["error"]
    assert "weight element(s)" in notes["fit_check_finite_nan_autograd"]["error"]
    for n in ("fit_checkpoint_resume_fused", "fit_checkpoint_resume_autograd"):
        assert {"first_ckpt_trainer", "ckpt_trainer", "first_model_pkl", "model_pkl"} <= set(rec["cases"][n]["digests"]) and notes[n]["epochs"] == 3
    called = {call[0] for c in rec["cases"].values() for call in c["trace"]}
    assert {"ltrx_fc_listnet_step", "ltrx_first_nonfinite", "ltrx_adam_step", "ltrx_listnet_fwd_bwd_cu", "ltrx_ndcg_at_cu",
            "ltrx_mrr_at_cu"} <= called                                                      # (the ragged loss and both ragged metrics)
    assert not set(rec["cases"]) & {n for k in ("calls", "rows", "step", "options") for n in recs[k]["cases"]}


CASE_SET = {name: key for key, (_, make) in G.SETS.items() for name in make()}


@pytest.mark.parametrize("name", sorted(CASE_SET))
def test_same_calls_same_bits(recs, proxy, name):
    want = recs[CASE_SET[name]]["cases"][name]
    trace, digests, notes = G.run_case(proxy, name)
    assert notes == want.get("notes", {}), (name, notes)
    assert len(trace) == len(want["trace"]), ([c[0] for c in trace], [c[0] for c in want["trace"]])
    for i, (got, exp) in enumerate(zip(trace, want["trace"])):
        assert got == exp, (name, i, got, exp)
    for key, sha in want["digests"].items():
        assert digests[key] == sha, (name, key)
