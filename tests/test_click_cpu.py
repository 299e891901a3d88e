"""No GPU: the click fixture has not drifted from the live reference, the numpy restatement of tests/click_cases.py equals it exactly,
``plan_of`` reads the reference's real objects, install(clicks=True) rebinds the four names, the host path of ``click_on_slates``
returns the reference's result and generator state, and ltrx_click_slates_cu refuses bad calls before any HIP call.  The
reference-dependent tests need the reference tree, as tests/test_rank_cpu.py does."""
import ctypes
import importlib
import inspect
import json
import os

import numpy as np
import pytest
import torch

from oracle.ref_loader import REFERENCE_ROOT, reference_available
from tests import click_cases as CC

needs_reference = pytest.mark.skipif(not reference_available(), reason="reference tree only exists in the build container")


@pytest.fixture(scope="module")
def g():
    return CC.golden()


@pytest.fixture()
def numpy_state():
    state = np.random.get_state()
    yield
    np.random.set_state(state)


def _reference_modules():
    from oracle.ref_loader import load_reference
    load_reference()
    cu = importlib.import_module("allrank.click_models.click_utils")
    ru = importlib.import_module("allrank.inference.inference_utils")
    rc = importlib.import_module("allrank.rank_and_click")
    return cu, ru, rc


# ------------------------------------------------------------------------------------------------------------------
# without the reference
# ------------------------------------------------------------------------------------------------------------------
def test_fixture_holds_every_case_and_its_inputs(g):
    assert {k.rsplit(".", 1)[0] for k in g} == set(CC.CASES)
    for name, c in CC.CASES.items():
        X, y = CC.inputs(name)
        assert np.array_equal(g[name + ".X"], X) and np.array_equal(g[name + ".y"], y), name
        assert np.array_equal(g[name + ".u"], CC.uniforms(name)), name
        assert g[name + ".clicks"].dtype == np.float32 and g[name + ".margin"].dtype == np.float64, name
    lens = CC.CASES["lds_edge.gauss"]["lens"]
    assert lens == [CC.LDS_LEN, CC.LDS_LEN + 1] and CC.CASES["long.gauss"]["lens"] == [300]
    assert len(CC.CASES["many_short"]["lens"]) == 300


@pytest.mark.parametrize("name", sorted(CC.CASES))
def test_restatement_equals_the_fixture(g, name, numpy_state):
    """clicks and generator state exactly, margins bit for bit: the sequential fp64 distance and the written-out quantile ARE what
    scipy's cdist and np.quantile computed"""
    c = CC.CASES[name]
    np.random.seed(c["seed"])
    clicks, margins = CC.restate_batch(c["model"], g[name + ".X"], g[name + ".y"])
    assert np.array_equal(clicks, g[name + ".clicks"]), name
    assert CC.state_digest() == str(g[name + ".state"]), name
    assert np.array_equal(margins.view(np.uint64), g[name + ".margin"].view(np.uint64)), name


@pytest.mark.parametrize("name", ["shipped.gauss.F3", "q0.25.lattice", "max_both.gauss", "plain.max.cascade"])
def test_the_specs_own_click_is_the_restatement(g, name, numpy_state):
    """the numpy ``click`` of the allrank_amd.clicks specs (what the host path runs for them) under MaskedRemainMasked's masking"""
    from allrank_amd import clicks as C
    c = CC.CASES[name]
    np.random.seed(c["seed"])
    got = C._host_clicks(torch.tensor(g[name + ".X"]), torch.tensor(g[name + ".y"]), CC.ours(c["model"]))
    assert np.array_equal(np.stack(got), g[name + ".clicks"]) and got[0].dtype == np.float32
    assert CC.state_digest() == str(g[name + ".state"])


def test_plan_of_reads_the_specs():
    from allrank_amd import clicks as C
    plan, why = C.plan_of(CC.ours(CC.SHIPPED))
    assert why == "" and plan == dict(kind="cascade", eta=1, threshold=2.0, max_candidates=-1, diverse=1, q=0.5, max_clicks=-1)
    plan, _ = C.plan_of(CC.ours(("max", 2, ("diverse", 0.25, ("max", 6, ("max", 4, ("relevant", 1)))))))
    assert plan == dict(kind="relevant", eta=None, threshold=1.0, max_candidates=4, diverse=1, q=0.25, max_clicks=2)
    plan, _ = C.plan_of(CC.ours(("max", 3, ("cascade", 0.5, 0))))
    assert plan["diverse"] == 0 and plan["max_clicks"] == 3 and plan["max_candidates"] == -1
    assert C.plan_of(C.MaxClicks(C.OnlyRelevant(1), None))[0]["max_clicks"] == -1
    for bad, word in [(C.Diverse(C.Diverse(C.OnlyRelevant(1), 0.5), 0.5), "inside a diverse"), (object(), "builtins.object"),
                      (C.Diverse(C.OnlyRelevant(1), 1.5), "outside"), (C.OnlyRelevant(0.1), "float32")]:
        plan, why = C.plan_of(bad)
        assert plan is None and word in why, (why, word)


def test_abi_refusals_and_size_query_run_without_a_gpu():
    from allrank_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.lib()
    fake = ctypes.c_void_p(4096)                               # never dereferenced: every check comes before the first HIP call
    q = ctypes.c_double(0.5)
    qp = ctypes.c_void_p(ctypes.addressof(q))

    def call(x=fake, y=fake, cu=fake, B=2, max_len=8, F=3, L=8, u=None, p=None, diverse=1, q=qp, out=fake, ws=None):
        return lib.ltrx_click_slates_cu(x, y, cu, None, B, max_len, F, L, u, p, 2.0, -1, diverse, q, -1, out, None, ws, None)

    for kw in (dict(x=None), dict(y=None), dict(cu=None), dict(out=None), dict(B=0), dict(F=0), dict(max_len=0), dict(L=7),
               dict(u=fake), dict(p=fake), dict(q=None)):
        assert call(**kw) == -1, kw
    for bad in (-0.01, 1.01, float("nan")):
        qb = ctypes.c_double(bad)
        assert call(q=ctypes.c_void_p(ctypes.addressof(qb))) == -1, bad
    big = _lib.MAX_SLATE_LEN + 1
    assert call(max_len=big, L=big, ws=fake) == -2                                     # diverse: LTRX_MAX_SLATE_LEN
    assert call(max_len=_lib.MAX_METRIC_SLATE_LEN + 1, L=_lib.MAX_METRIC_SLATE_LEN + 1, diverse=0, q=None) == -2
    assert call(max_len=CC.LDS_LEN + 1, L=CC.LDS_LEN + 1, ws=None) == -1               # a slab is needed and ws is NULL
    # the size query: 0 without `diverse` and while the distances fit LDS, min(B, slab workgroups) slabs of pairs beyond
    slabs = CC.header_constant("LTRX_CLICK_SLAB_WORKGROUPS")
    size = lib.ltrx_click_workspace_bytes
    assert size(64, 2048, 0) == 0 and size(64, CC.LDS_LEN, 1) == 0 and size(0, 2048, 1) == 0 and size(64, 0, 1) == 0
    n = CC.LDS_LEN + 1
    assert size(3, n, 1) == 3 * (n * (n - 1) // 2) * 8
    assert size(slabs, 2048, 1) == size(slabs + 1, 2048, 1) == size(1 << 20, 2048, 1) == slabs * (2048 * 2047 // 2) * 8


def test_click_slates_cu_states_the_call_by_header_name():
    from tests.test_kernel_calls_cpu import NAMES, Recorder, _expect, ST, f32, i32
    from allrank_amd import clicks as C
    B, L, F, ml = 3, 7, 12, 5
    x, y, cu, order, out = f32(B, L, F), f32(B, L), i32(B + 1), i32(B), f32(B, L)
    u, table, mg, ws = torch.zeros(11, dtype=torch.float64), torch.zeros(L, dtype=torch.float64), torch.zeros(B, dtype=torch.float64), f32(64)
    plan = dict(kind="cascade", eta=1, threshold=2.0, max_candidates=4, diverse=1, q=0.25, max_clicks=6)
    rec = Recorder()
    C.click_slates_cu(rec, ST, x, y, cu, order, B, ml, out, plan, u, table, mg, ws)
    (name, args), = rec.calls
    q_addr = args[NAMES[name].index("q_host")]                 # the address of a local double: only its slot can be expected
    assert isinstance(q_addr, int) and q_addr != 0
    _expect(rec, "ltrx_click_slates_cu", x=x.data_ptr(), y=y.data_ptr(), cu_seqlens=cu.data_ptr(), slate_order=order.data_ptr(), B=B,
            max_len=ml, F=F, L=L, u=u.data_ptr(), observe_p=table.data_ptr(), threshold=2.0, max_candidates=4, diverse=1, q_host=q_addr,
            max_clicks=6, clicks_out=out.data_ptr(), margin_out=mg.data_ptr(), ws=ws.data_ptr(), stream=ST.value)


def test_host_path_serves_a_model_without_a_plan_and_says_why(numpy_state):
    """no reference installed: the per-slate loop over ``click_model.click`` with the masking restated"""
    from allrank_amd import clicks as C

    class FirstTwo(object):
        def click(self, documents):
            c = np.zeros(len(documents[1]), dtype=bool)
            c[:2] = True
            return c

    X, y = CC.inputs("plain.relevant")
    Xt, yt = torch.tensor(X), torch.tensor(y)
    kept_X, clicks = C.click_on_slates((Xt, yt), FirstTwo(), include_empty=True)
    assert C.last_run["engine"] == "host" and "FirstTwo" in C.last_run["reason"]
    assert len(clicks) == len(CC.LENS) and all(v.dtype == np.float32 and v.shape == (65,) for v in clicks)
    for b, n in enumerate(CC.LENS):
        assert (clicks[b][:min(n, 2)] == 1).all() and (clicks[b][min(n, 2):n] == 0).all() and (clicks[b][n:] == -1).all()
        assert kept_X[b] is not None and torch.equal(kept_X[b], Xt[b])
    kept_X, clicks = C.click_on_slates((Xt, yt), FirstTwo(), include_empty=False)
    assert len(clicks) == len(CC.LENS) - 1                     # the empty slate got no click
    with pytest.raises(ValueError):                            # nothing kept: the reference's exception type
        C.click_on_slates((Xt[:1], yt[:1]), FirstTwo(), include_empty=False)


def test_metrics_on_clicked_slates_host_form(monkeypatch):
    """without a GPU the generator computes the reference's quantities on the host (on a GPU: tests/test_gpu_click.py)"""
    from allrank_amd import clicks as C
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    c = [np.array([1, 0, 1, 0, -1], dtype=np.float32), np.array([0, 0, -1], dtype=np.float32), np.array([0, 1, 1], dtype=np.float32)]
    out = list(C.metrics_on_clicked_slates(([None] * 3, c)))
    assert [d["slate_length"] for d in out] == [5, 3, 3] and [int(d["no_of_clicks"]) for d in out] == [2, 0, 2]
    assert list(out[0]) == ["slate_length", "no_of_clicks", "dcg", "ndcg"]
    d0 = 1.0 + 1.0 / np.log2(4.0)
    assert abs(out[0]["dcg"] - d0) <= 1e-6 and abs(out[0]["ndcg"] - d0 / (1.0 + 1.0 / np.log2(3.0))) <= 1e-6
    assert out[1]["dcg"] == 0.0 and out[1]["ndcg"] == 1.0


# ------------------------------------------------------------------------------------------------------------------
# with the reference
# ------------------------------------------------------------------------------------------------------------------
@needs_reference
def test_committed_click_golden_equals_the_live_reference(g, numpy_state):
    built = importlib.import_module("tests.golden.make_golden_clicks").build()
    assert list(built) == ["click_golden.npz"]
    fresh = built["click_golden.npz"]
    assert set(g) == set(fresh), sorted(set(g) ^ set(fresh))
    for k in g:
        a, b = np.asarray(g[k]), np.asarray(fresh[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (k, a.shape, b.shape, a.dtype, b.dtype)
        if k.endswith(".margin"):
            assert np.all(np.abs(a - b) <= 1e-12 * np.abs(a)), k
        else:
            assert (a == b).all(), k


@needs_reference
def test_plan_of_reads_the_references_objects():
    from allrank_amd import clicks as C
    _reference_modules()
    from allrank.click_models.base import FixedClickModel, MultipleClickModel, ConditionedClickModel, RandomClickModel
    from allrank.click_models.duplicate_aware import EverythingButDuplicatesClickModel
    from allrank.config import NameArgsConfig
    from allrank.utils.config_utils import instantiate_from_recursive_name_args
    with open(os.path.join(REFERENCE_ROOT, "scripts", "local_config_click_model.json")) as fh:
        shipped = instantiate_from_recursive_name_args(NameArgsConfig(**json.load(fh)["click_model"]))
    plan, why = C.plan_of(shipped)
    assert why == "" and plan == C.plan_of(CC.ours(CC.SHIPPED))[0]
    for name, c in CC.CASES.items():
        assert C.plan_of(CC.theirs(c["model"])) == C.plan_of(CC.ours(c["model"])), name
    inner = CC.theirs(("relevant", 1))
    for bad in (RandomClickModel(2), FixedClickModel([0]), MultipleClickModel([inner], [1.0]), ConditionedClickModel([inner], np.all),
                EverythingButDuplicatesClickModel(0.5), CC.theirs(("diverse", 0.5, ("diverse", 0.5, ("relevant", 1))))):
        plan, why = C.plan_of(bad)
        assert plan is None and why, type(bad)
    assert "RandomClickModel" in C.plan_of(RandomClickModel(2))[1]


@needs_reference
def test_install_clicks_rebinds_the_four_names_and_uninstall_restores():
    import allrank_amd
    from allrank_amd import clicks as C
    cu, ru, rc = _reference_modules()
    ref_c, ref_m, ref_r = cu.click_on_slates, ru.metrics_on_clicked_slates, ru.rank_slates
    assert rc.click_on_slates is ref_c and rc.metrics_on_clicked_slates is ref_m
    names = {"allrank.click_models.click_utils.click_on_slates", "allrank.rank_and_click.click_on_slates",
             "allrank.inference.inference_utils.metrics_on_clicked_slates", "allrank.rank_and_click.metrics_on_clicked_slates"}
    for kw in (dict(), dict(inference=True)):                  # neither rides on the other opt-in
        done = allrank_amd.install(data=False, **kw)
        try:
            assert not names & set(done)
            assert cu.click_on_slates is ref_c and rc.click_on_slates is ref_c
            assert ru.metrics_on_clicked_slates is ref_m and rc.metrics_on_clicked_slates is ref_m
        finally:
            allrank_amd.uninstall()
    plain = allrank_amd.install(data=False)
    allrank_amd.uninstall()
    done = allrank_amd.install(data=False, clicks=True)
    try:
        assert [n for n in done if n not in names] == plain and names <= set(done)
        assert cu.click_on_slates is C.click_on_slates and rc.click_on_slates is C.click_on_slates
        assert ru.metrics_on_clicked_slates is C.metrics_on_clicked_slates and rc.metrics_on_clicked_slates is C.metrics_on_clicked_slates
        assert ru.rank_slates is ref_r and rc.rank_slates is ref_r
        assert inspect.signature(C.click_on_slates) == inspect.signature(ref_c)
        assert inspect.signature(C.metrics_on_clicked_slates) == inspect.signature(ref_m)
        assert C._reference == {"click_on_slates": ref_c, "metrics_on_clicked_slates": ref_m}
    finally:
        allrank_amd.uninstall()
    assert cu.click_on_slates is ref_c and rc.click_on_slates is ref_c
    assert ru.metrics_on_clicked_slates is ref_m and rc.metrics_on_clicked_slates is ref_m and not C._reference
    assert inspect.signature(allrank_amd.install).parameters["clicks"].default is False
    ours, ref = inspect.signature(C.click_on_slates), inspect.signature(ref_c)
    assert [(p.name, p.kind, p.default) for p in ours.parameters.values()] == [(p.name, p.kind, p.default) for p in ref.parameters.values()]


@needs_reference
def test_host_path_returns_the_references_result_and_generator_state(numpy_state):
    """a model without a plan (RandomClickModel draws from the global generator), installed and not installed"""
    import allrank_amd
    from allrank_amd import clicks as C
    cu, _, _ = _reference_modules()
    from allrank.click_models.base import RandomClickModel
    X, y = CC.inputs("plain.relevant")
    Xt, yt = torch.tensor(X[2:]), torch.tensor(y[2:])          # (slates of at least two items: the model clicks twice)
    np.random.seed(5)
    want_X, want = cu.click_on_slates((Xt, yt), RandomClickModel(2), include_empty=False)
    want_state = CC.state_digest()
    for installed in (False, True):
        if installed:
            allrank_amd.install(data=False, clicks=True)
        try:
            np.random.seed(5)
            got_X, got = C.click_on_slates((Xt, yt), RandomClickModel(2), include_empty=False)
        finally:
            allrank_amd.uninstall()
        assert C.last_run["engine"] == "host" and "RandomClickModel" in C.last_run["reason"]
        assert CC.state_digest() == want_state
        assert len(got) == len(want) and all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(got, want))
        assert all(torch.equal(a, b) for a, b in zip(got_X, want_X))


def _run_entry(entry, tmp_path, name, cfg, model_path):
    import sys
    argv = sys.argv
    sys.argv = ["rank_and_click", "--job-dir", str(tmp_path / name), "--run-id", "r", "--config-file-name", str(cfg),
                "--input-model-path", str(model_path), "--roles", "vali,test"]
    try:
        entry.run()
    finally:
        sys.argv = argv
    out = tmp_path / name / "results" / "r"
    return {f: (out / f).read_bytes() for f in sorted(os.listdir(out)) if f.endswith((".txt", ".csv"))}


@needs_reference
def test_unmodified_rank_and_click_writes_the_same_files_under_install(tmp_path, numpy_state):
    """the reference's second entry point, unmodified, plain and under install(inference=True, clicks=True): the same {role}.txt,
    {role}_metrics.csv and {role}_metrics_mean.csv for its fixed seed.  On a machine without a GPU both of our functions take their
    host paths (the module ranking, the kept original click_on_slates), which is what this test can hold: the wiring of the four names
    through a whole run.  The device paths are held to the same fixtures in tests/test_gpu_click.py."""
    import logging
    import allrank_amd
    from allrank_amd import clicks as C
    _, _, entry = _reference_modules()
    from allrank.models.model import make_model
    from allrank.config import Config
    rs = np.random.RandomState(3)
    data = tmp_path / "data"
    data.mkdir()
    for role in ("vali", "test"):
        with open(data / (role + ".txt"), "w") as fh:
            for qid in range(6):
                for _ in range(int(rs.randint(2, 9))):
                    feats = " ".join("%d:%.4f" % (k + 1, v) for k, v in enumerate(rs.standard_normal(5)))
                    fh.write("%d qid:%d %s\n" % (rs.randint(0, 5), qid, feats))
    cfg = {"model": {"fc_model": {"sizes": [8], "input_norm": False, "activation": None, "dropout": 0.0},
                     "transformer": {"N": 1, "d_ff": 8, "h": 1, "positional_encoding": None, "dropout": 0.0},
                     "post_model": {"output_activation": None, "d_output": 1}},
           "data": {"path": str(data), "validation_ds_role": "vali", "num_workers": 0, "batch_size": 4, "slate_length": 8},
           "optimizer": {"name": "Adam", "args": {"lr": 0.001}}, "lr_scheduler": {"name": "StepLR", "args": {"step_size": 3, "gamma": 0.5}},
           "training": {"epochs": 1, "early_stopping_patience": 1, "gradient_clipping_norm": None}, "val_metric": "ndcg_5",
           "metrics": ["ndcg_5"], "loss": {"name": "listNet", "args": {}},
           "click_model": {"name": "allrank.click_models.cascade_models.DiverseClicksModel",
                           "args": {"inner_click_model": {"name": "allrank.click_models.cascade_models.BaseCascadeModel",
                                                          "args": {"eta": 0.5, "threshold": 1}}, "q_percentile": 0.5}}}
    cfg_path = tmp_path / "config.json"
    cfg_path.write_text(json.dumps(cfg))
    torch_state = torch.get_rng_state()                        # (restored below: run() seeds torch and numpy with 42)
    torch.manual_seed(0)
    c = Config.from_json(str(cfg_path))
    import attr
    model = make_model(n_features=5, **attr.asdict(c.model, recurse=False))
    model_path = tmp_path / "model.pkl"
    torch.save(model.state_dict(), str(model_path))
    handlers = list(logging.getLogger().handlers)
    try:
        want = _run_entry(entry, tmp_path, "plain", cfg_path, model_path)
        allrank_amd.install(losses=False, metrics=False, model=False, data=False, inference=True, clicks=True)
        try:
            got = _run_entry(entry, tmp_path, "installed", cfg_path, model_path)
        finally:
            allrank_amd.uninstall()
    finally:
        logging.getLogger().handlers[:] = handlers
        torch.set_rng_state(torch_state)
    assert C.last_run["engine"] in ("host", "device")
    assert sorted(want) == ["test.txt", "test_metrics.csv", "test_metrics_mean.csv", "vali.txt", "vali_metrics.csv", "vali_metrics_mean.csv"]
    assert got == want
