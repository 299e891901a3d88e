"""ltrx_click_slates_cu and allrank_amd.clicks on the GPU against tests/golden/click_golden.npz: what the reference's own
``click_on_slates`` returned on CPU for the cases of tests/click_cases.py (integer-lattice data with exact ties, gaussian data with
the generator's gap condition).  Clicks are held EXACTLY; margins to 1e-12 relative (the fp64 summation bound F * 2^-53 is 1.1e-13 at
F = 1024; one rounding each for the root and the interpolation sit well inside the rest), and whether they are bit-equal is printed."""
import numpy as np
import pytest
import torch

from tests import click_cases as CC
from tests import rank_cases as RC

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 7.0
bit_equal_margins = {}


@pytest.fixture(scope="module")
def g():
    return CC.golden()


@pytest.fixture()
def numpy_state():
    state = np.random.get_state()
    yield
    np.random.set_state(state)


def _launch(g, name, want_margin=True, order="longest"):
    """one direct kernel call on a stored case with the stored uniforms: (clicks buffer [N + 2, L] with a guard row either side,
    margins buffer [N + 2] likewise or None)"""
    from allrank_amd import _lib as LB, clicks as C
    c = CC.CASES[name]
    plan, why = C.plan_of(CC.ours(c["model"]))
    assert plan is not None, why
    X, y, lens = g[name + ".X"], g[name + ".y"], np.asarray(c["lens"], dtype=np.int64)
    N, L, _ = X.shape
    xb, yb = torch.tensor(X, device=DEV), torch.tensor(y, device=DEV)
    cu = torch.tensor(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), device=DEV)
    orders = {"longest": np.argsort(-lens, kind="stable"), "reversed": np.arange(N)[::-1].copy(), None: None}
    od = None if orders[order] is None else torch.tensor(orders[order].astype(np.int32), device=DEV)
    u = table = None
    if plan["kind"] == "cascade":
        u = torch.tensor(g[name + ".u"], dtype=torch.float64, device=DEV)
        table = torch.tensor(1 / np.arange(1, L + 1) ** plan["eta"], dtype=torch.float64, device=DEV)
    buf = torch.full((N + 2, L), GUARD, dtype=torch.float32, device=DEV)
    mbuf = torch.full((N + 2,), GUARD, dtype=torch.float64, device=DEV) if want_margin else None
    max_len = max(int(lens.max()), 1)
    nbytes = LB.lib().ltrx_click_workspace_bytes(N, max_len, plan["diverse"])
    assert (nbytes > 0) == (plan["diverse"] == 1 and max_len > CC.LDS_LEN)
    ws = torch.full((nbytes + 64,), 0x5A, dtype=torch.uint8, device=DEV) if nbytes else None
    C.click_slates_cu(LB.lib(), LB.launch_stream(DEV), xb, yb, cu, od, N, max_len, buf[1:N + 1], plan, u, table,
                      None if mbuf is None else mbuf[1:N + 1], ws)
    torch.cuda.synchronize()
    if ws is not None:
        assert (ws[nbytes:] == 0x5A).all(), "the workspace was written beyond its size query"
    return buf.cpu().numpy(), None if mbuf is None else mbuf.cpu().numpy()


def _check_buffer(buf, want, lens):
    assert (buf[0] == GUARD).all() and (buf[-1] == GUARD).all(), "a write outside clicks_out[B, L]"
    got = buf[1:-1]
    for b, n in enumerate(lens):
        assert (got[b, n:] == -1).all(), b
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]


@pytest.mark.parametrize("name", sorted(CC.CASES))
def test_kernel_gives_the_stored_clicks_and_margins(g, name):
    buf, mbuf = _launch(g, name)
    _check_buffer(buf, g[name + ".clicks"], CC.CASES[name]["lens"])
    assert mbuf[0] == GUARD and mbuf[-1] == GUARD
    got, want = mbuf[1:-1], g[name + ".margin"]
    err = np.abs(got - want) / np.where(want == 0, 1.0, np.abs(want))
    bit_equal_margins[name] = bool(np.array_equal(got.view(np.uint64), want.view(np.uint64)))
    print("%s: worst relative margin error %.3g, bit-equal %s" % (name, float(err.max()), bit_equal_margins[name]))
    assert float(err.max()) <= 1e-12, (name, float(err.max()))


@pytest.mark.parametrize("name", sorted(CC.CASES))
def test_without_margin_out_the_clicks_are_unchanged(g, name):
    """margin_out NULL: slates with fewer than two candidates skip their distance work"""
    buf, _ = _launch(g, name, want_margin=False)
    _check_buffer(buf, g[name + ".clicks"], CC.CASES[name]["lens"])


@pytest.mark.parametrize("name", ["shipped.gauss.F3", "q0.5.lattice", "max_both.gauss", "many_short", "lds_edge.gauss", "plain.max.cascade"])
def test_result_does_not_depend_on_the_launch_order(g, name):
    for order in (None, "reversed"):
        buf, mbuf = _launch(g, name, order=order)
        _check_buffer(buf, g[name + ".clicks"], CC.CASES[name]["lens"])
        assert np.allclose(mbuf[1:-1], g[name + ".margin"], rtol=1e-12, atol=0)


def test_all_margins_bit_equal_report():
    """(a report, after the parametrised test above in file order: which cases' margins were bit-equal to np.quantile of cdist)"""
    off = sorted(k for k, v in bit_equal_margins.items() if not v)
    print("margins bit-equal in %d of %d cases; not bit-equal: %s" % (len(bit_equal_margins) - len(off), len(bit_equal_margins), off))


E2E = ["shipped.gauss.F3", "shipped.lattice.F136", "q0.5.gauss", "eta05.thr-1.gauss", "max_both.lattice", "many_short", "lds_edge.gauss",
       "long.gauss", "plain.relevant"]


@pytest.mark.parametrize("name", E2E)
@pytest.mark.parametrize("source", ["cpu", "device"])
def test_click_on_slates_equals_the_fixture_end_to_end(g, name, source, monkeypatch, numpy_state):
    from allrank_amd import clicks as C
    c = CC.CASES[name]
    X, y = torch.tensor(g[name + ".X"]), torch.tensor(g[name + ".y"])
    if source == "device":
        X, y = X.to(DEV), y.to(DEV)
    want = g[name + ".clicks"]
    some = [s for s in range(want.shape[0]) if (want[s] > 0).any()]
    for chunk in (1, 1 << 40):                                 # one slate per launch, and the whole set in one
        monkeypatch.setattr(C, "CHUNK_BYTES", chunk)
        for include_empty in (True, False):
            np.random.seed(c["seed"])
            kept_X, clicks = C.click_on_slates((X, y), CC.ours(c["model"]), include_empty)
            assert C.last_run == {"engine": "device", "reason": ""}
            assert CC.state_digest() == str(g[name + ".state"])
            rows = list(range(want.shape[0])) if include_empty else some
            assert len(clicks) == len(rows) == len(kept_X)
            for s, v, xs in zip(rows, clicks, kept_X):
                assert isinstance(v, np.ndarray) and v.dtype == np.float32 and np.array_equal(v, want[s]), (s, chunk)
                assert xs.device == X.device and torch.equal(xs, X[s])


def test_nothing_kept_raises_the_references_exception_type(g):
    from allrank_amd import clicks as C
    X, y = torch.tensor(g["plain.relevant.X"][:1]), torch.tensor(g["plain.relevant.y"][:1])         # the empty slate
    with pytest.raises(ValueError):
        C.click_on_slates((X, y), C.OnlyRelevant(2), include_empty=False)
    assert C.last_run["engine"] == "device"


def test_host_path_on_a_gpu_machine_says_why(g, numpy_state):
    """a model without a plan, and a slate with padding between its valid items: the host path, the restatement's result"""
    from allrank_amd import clicks as C

    class Wrapped(object):                                     # an unknown class around a known model
        def __init__(self, inner):
            self.inner = inner

        def click(self, documents):
            return self.inner.click(documents)

    name = "eta05.thr0.gauss"
    c = CC.CASES[name]
    X, y = torch.tensor(g[name + ".X"]), torch.tensor(g[name + ".y"])
    np.random.seed(c["seed"])
    _, clicks = C.click_on_slates((X.to(DEV), y.to(DEV)), Wrapped(CC.ours(c["model"])), include_empty=True)
    assert C.last_run["engine"] == "host" and "Wrapped" in C.last_run["reason"]
    assert np.array_equal(np.stack(clicks), g[name + ".clicks"]) and CC.state_digest() == str(g[name + ".state"])

    yh = g[name + ".y"].copy()
    yh[-1, 3] = -1                                             # padding inside the longest slate
    np.random.seed(c["seed"])
    want, _ = CC.restate_batch(c["model"], g[name + ".X"], yh)
    state = CC.state_digest()
    np.random.seed(c["seed"])
    _, clicks = C.click_on_slates((X, torch.tensor(yh)), CC.ours(c["model"]), include_empty=True)
    assert C.last_run["engine"] == "host" and "padding between" in C.last_run["reason"]
    assert np.array_equal(np.stack(clicks), want) and CC.state_digest() == state


def _restated_metrics(c):
    """dcg and ndcg of one click vector in ranked order (gain 2^y - 1, log2 discount, filler 1.0), fp64"""
    gains = np.where(c > 0, 2.0 ** np.maximum(c, 0).astype(np.float64) - 1.0, 0.0)
    disc = 1.0 / np.log2(np.arange(len(c)) + 2.0)
    dcg, ideal = float((gains * disc).sum()), float((np.sort(gains)[::-1] * disc).sum())
    return dcg, (dcg / ideal if ideal > 0 else 1.0)


def test_metrics_on_clicked_slates_equal_the_restated_metrics(g):
    """slates of two lengths in one call (grouped by length), each against the per-slate restatement: 1e-5, the metric contract"""
    from allrank_amd import clicks as C
    vectors = list(g["q0.5.lattice.clicks"]) + list(g["long.gauss.clicks"]) + list(g["shipped.gauss.F3.clicks"])
    out = list(C.metrics_on_clicked_slates(([None] * len(vectors), vectors)))
    assert len(out) == len(vectors)
    for d, v in zip(out, vectors):
        assert list(d) == ["slate_length", "no_of_clicks", "dcg", "ndcg"]
        assert d["slate_length"] == len(v) and d["no_of_clicks"] == int((v > 0).sum())
        dcg, ndcg = _restated_metrics(v)
        assert abs(d["dcg"] - dcg) <= 1e-5 * max(1.0, abs(dcg)) and abs(d["ndcg"] - ndcg) <= 1e-5, (d, dcg, ndcg)


def test_ranked_batches_feed_the_click_call_on_the_device(numpy_state):
    """inference.rank_batches output (device tensors, views of the ranker's buffers) straight into click_on_slates == ranking, then
    clicking through the restatement"""
    from allrank_amd import clicks as C, inference as EI
    rg = RC.golden()
    model = RC.golden_model(rg, DEV)
    xb, yb = torch.tensor(rg["x"]), torch.tensor(rg["y"])
    spec = ("diverse", 0.5, ("cascade", 0.5, 1))
    (xr, yr), = list(EI.rank_batches(model, [(xb, yb)], xb.shape[0], xb.shape[1]))
    assert xr.is_cuda and yr.is_cuda
    np.random.seed(3)
    _, clicks = C.click_on_slates((xr, yr), CC.ours(spec), include_empty=True)
    assert C.last_run["engine"] == "device"
    state = CC.state_digest()
    np.random.seed(3)
    want, _ = CC.restate_batch(spec, xr.cpu().numpy(), yr.cpu().numpy())
    assert np.array_equal(np.stack(clicks), want) and CC.state_digest() == state
    assert (want == 1).any() and (want == 0).any()
