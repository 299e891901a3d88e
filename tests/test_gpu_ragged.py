"""The ragged (cu_seqlens) losses and metrics on the GPU (-m gpu) against the fp64 oracle on the padded grid.

One batch (tests/ragged_cases.py): slates of 0, 1, 2, 3, 5, 31, 32, 33, 64, 100, 255, 256, 257 items, labels 0..4, one slate of zero
labels, exact ties in scores and labels, at score scales 1 and 30.  Bars: those of the padded kernels' tests -- value ``close``
(1e-5), gradient ``grad_close`` (2e-4 of the largest reference entry), argsorts and pair counts exact.  The entrywise bar of the
ragged listNet, approxNDCG and lambdaLoss calls lives in tests/test_gpu_listwise_contract.py."""
import ctypes

import numpy as np
import pytest
import torch

from tests import ragged_cases as RC
from tests.cases import close, grad_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCALES = (1, 30)


def _t(a, dtype=None, rg=False):
    return torch.tensor(np.asarray(a), device=DEV, dtype=dtype, requires_grad=rg)


@pytest.fixture(scope="module")
def exp():
    """scale -> the oracle's values on the grid of width 257, computed once"""
    return {sc: RC.expected(sc) for sc in SCALES}


def _order_of(cu):
    return _t(np.argsort(-np.diff(cu), kind="stable").astype(np.int32))


class _Abi(object):
    """the five *_cu entry points called directly, with every optional output"""

    def __init__(self, s, y, cu, max_len, order=None):
        from allrank_amd import _lib
        self.L, self.lib = _lib, _lib.lib()
        self.s, self.y, self.cu = _t(s, torch.float32), _t(y, torch.float32), _t(cu, torch.int32)
        self.B, self.n, self.max_len, self.order = len(cu) - 1, int(cu[-1]), int(max_len), order
        self.st = _lib.stream_of(self.s)

    def _out(self, *shape, dtype=torch.float32):
        return torch.full(shape, -777, dtype=dtype, device=DEV)         # a value no output can keep by accident

    def _ws(self, nbytes):
        return torch.empty(max(int(nbytes), 64), dtype=torch.uint8, device=DEV)

    def loss(self, kind, **kw):
        """(loss, grad[n], per_slate[B] or None, pair count or None, order[n] or None)"""
        P, lib, B = self.L.ptr, self.lib, self.B
        loss, grad, per = self._out(1), self._out(max(self.n, 1)), self._out(B)
        head = (P(self.s), P(self.y), P(self.cu), P(self.order), B, self.max_len, 1e-10)
        if kind == "listnet":
            ws = self._ws(lib.ltrx_listnet_workspace_bytes(B, self.max_len))
            rc = lib.ltrx_listnet_fwd_bwd_cu(*head, float(B), P(loss), P(per), P(grad), P(ws), self.st)
            extra = (per.cpu().numpy().astype(np.float64), None, None)
        elif kind == "approxndcg":
            ws = self._ws(lib.ltrx_approxndcg_workspace_bytes(B, self.max_len))
            rc = lib.ltrx_approxndcg_fwd_bwd_cu(*head, float(kw.get("alpha", 1.0)), float(B), P(loss), P(per), P(grad), P(ws), self.st)
            extra = (per.cpu().numpy().astype(np.float64), None, None)
        else:
            from allrank_amd.losses import _SCHEMES
            sch, k, red, lg = kw["case"]
            cnt, perm = self._out(1), self._out(max(self.n, 1), dtype=torch.int64)
            ws = self._ws(lib.ltrx_lambdaloss_workspace_bytes(B, self.max_len))
            rc = lib.ltrx_lambdaloss_fwd_bwd_cu(*head, _SCHEMES[sch], 0 if k is None else k, RC.LAMBDA_KW["sigma"], RC.LAMBDA_KW["mu"],
                                                0 if red == "sum" else 1, 0 if lg == "binary" else 1, None, P(loss), P(cnt), P(grad),
                                                P(perm), P(ws), self.st)
            extra = (None, float(cnt.item()), perm[:self.n].cpu().numpy())
        self.L.check(rc, kind)
        return (float(loss.item()), grad[:self.n].cpu().numpy().astype(np.float64)) + extra

    def metrics(self, ats=RC.ATS, filler=1.0):
        P, lib, B = self.L.ptr, self.lib, self.B
        arr = (ctypes.c_int * len(ats))(*ats)
        nd, dc, mr = self._out(B, len(ats)), self._out(B, len(ats)), self._out(B, len(ats))
        perm = self._out(max(self.n, 1), dtype=torch.int64)
        self.L.check(lib.ltrx_ndcg_at_cu(P(self.s), P(self.y), P(self.cu), P(self.order), B, self.max_len, arr, len(ats), float(filler),
                                         P(nd), P(dc), P(perm), None, self.st), "ndcg_at_cu")
        ws = self._ws(lib.ltrx_mrr_workspace_bytes(B, self.max_len, len(ats)))
        self.L.check(lib.ltrx_mrr_at_cu(P(self.s), P(self.y), P(self.cu), P(self.order), B, self.max_len, arr, len(ats), P(mr), P(ws),
                                        self.st), "mrr_at_cu")
        return nd.cpu().numpy(), dc.cpu().numpy(), perm[:self.n].cpu().numpy(), mr.cpu().numpy()


def _check_loss(got, want, what):
    loss, grad = got[:2]
    print(what, "loss", loss, "oracle", want[0], "max |grad err|", float(np.abs(grad - want[1]).max()), "max |grad|",
          float(np.abs(want[1]).max()))
    assert np.isfinite(loss) and np.isfinite(grad).all(), what
    assert close(loss, want[0]), (what, loss, want[0])
    assert grad_close(grad, want[1]), what


@pytest.mark.parametrize("scale", SCALES)
def test_listnet_and_approxndcg_value_gradient_and_per_slate(scale, exp):
    e = exp[scale]
    abi = _Abi(e["s"], e["y"], e["cu"], 257)
    for kind in ("listnet", "approxndcg"):
        got = abi.loss(kind)
        _check_loss(got, e[kind], "%s x%d" % (kind, scale))
        assert close(got[2], e[kind][2]), (kind, got[2], e[kind][2])
        assert got[2][0] == 0.0                                           # the empty slate


@pytest.mark.parametrize("scale", SCALES)
def test_lambdaloss_all_schemes_value_gradient_pair_count_and_order(scale, exp):
    e = exp[scale]
    abi = _Abi(e["s"], e["y"], e["cu"], 257)
    for c in RC.LAMBDA_CASES:
        want = e[("lambda",) + c]
        got = abi.loss("lambdaloss", case=c)
        _check_loss(got, want, "lambdaloss %s x%d" % (c, scale))
        assert got[3] == want[2], (c, got[3], want[2])                    # selected pairs, exact
        assert np.array_equal(got[4], want[3]), c                         # stable argsort as in-slate indices, bit-exact


@pytest.mark.parametrize("scale", SCALES)
def test_metrics_order_filler_and_cutoffs_beyond_the_slate(scale, exp):
    e = exp[scale]
    abi = _Abi(e["s"], e["y"], e["cu"], 257)
    for key, filler in (("metrics", 1.0), ("metrics_f0", 0.25)):
        nd, dc, perm, mr = abi.metrics(filler=filler)
        wnd, wdc, wperm, wmr = e[key]
        assert close(nd, wnd) and close(dc, wdc) and close(mr, wmr), key
        assert np.array_equal(perm, wperm), key
        assert np.all(nd[0] == np.float32(filler)) and np.all(nd[RC.ZERO_LABEL_SLATE] == np.float32(filler)) and not dc[0].any()


def test_mrr_of_a_batch_without_a_relevant_item_is_all_zero(exp):
    e = exp[1]
    z = np.zeros_like(e["y"])
    abi = _Abi(e["s"], z, e["cu"], 257)
    mr = abi.metrics()[3]
    sg, yg = RC.grids(e["s"], z, e["cu"], 257)
    assert not RC.metrics_expected(sg, yg, e["cu"])[3].any()
    assert mr.shape == (len(RC.LENGTHS), len(RC.ATS)) and not mr.any()


@pytest.mark.parametrize("scale", SCALES)
def test_results_do_not_depend_on_slate_order_or_on_a_larger_max_len(scale, exp):
    """slate_order given or not: identical bits (a slate's workgroup computes the same thing wherever it is launched; the batch sums
    run over slates in index order).  max_len 921 instead of 257 moves the carve of the work arrays, and max_len may move the
    metric kernel's thread count: within ``close`` of each other and of the oracle."""
    e = exp[scale]
    base = _Abi(e["s"], e["y"], e["cu"], 257)
    cases = [("listnet", {}), ("approxndcg", {}), ("lambdaloss", dict(case=("ndcgLoss2PP_scheme", 5, "mean", "natural"))),
             ("lambdaloss", dict(case=("ndcgLoss1_scheme", None, "sum", "binary")))]
    for other in (_Abi(e["s"], e["y"], e["cu"], 257, order=_order_of(e["cu"])), _Abi(e["s"], e["y"], e["cu"], 921),
                  _Abi(e["s"], e["y"], e["cu"], 921, order=_order_of(e["cu"]))):
        for kind, kw in cases:
            a, b = base.loss(kind, **kw), other.loss(kind, **kw)
            want = e[kind] if kind != "lambdaloss" else e[("lambda",) + kw["case"]]
            _check_loss(b, want, "%s max_len %d order %s" % (kind, other.max_len, other.order is not None))
            assert close(b[0], a[0]) and close(b[1], a[1]), (kind, other.max_len)
            if other.max_len == 257:
                assert b[0] == a[0] and np.array_equal(b[1], a[1]), kind
            assert b[3] == a[3] and (a[4] is None or np.array_equal(a[4], b[4])), kind          # pair count, argsort: exact
            assert a[2] is None or close(b[2], a[2]), kind
        (nd, dc, perm, mr), (nd2, dc2, perm2, mr2) = base.metrics(), other.metrics()
        assert close(nd2, nd) and close(dc2, dc) and np.array_equal(perm2, perm) and np.array_equal(mr2, mr)
        if other.max_len == 257:                                  # (a max_len on the other side of the metric kernel's thread rule: another scan order)
            assert np.array_equal(nd2, nd) and np.array_equal(dc2, dc)


def _one_long(kind, max_len, seed):
    """two slates, one of max_len items and one of 7: the work arrays of a slate this long live in the call's workspace"""
    from allrank_amd import _lib
    s, y, cu = RC.make_batch(1, seed=seed, lengths=(max_len, 7))
    fn = getattr(_lib.lib(), "ltrx_%s_workspace_bytes" % kind)
    assert fn(2, max_len) > fn(2, max_len // 2) + 2 * 4 * max_len          # the workspace form: per-slate work arrays behind the results
    abi = _Abi(s, y, cu, max_len, order=_t(np.array([0, 1], np.int32)))
    # the oracle slate by slate (its pair tensors are quadratic in the grid width): the batch is the mean / sum of the two
    parts = []
    for b in range(2):
        sb, yb = s[cu[b]:cu[b + 1]][None].astype(np.float64), y[cu[b]:cu[b + 1]][None].astype(np.float64)
        parts.append((sb, yb, np.array([0, cu[b + 1] - cu[b]], np.int32)))
    return abi, parts


def test_approxndcg_workspace_form_at_max_len_5900():
    abi, parts = _one_long("approxndcg", 5900, 31)
    res = [RC.approxndcg_expected(*p) for p in parts]
    want = (sum(r[0] for r in res) / 2, np.concatenate([r[1] for r in res]) / 2, np.concatenate([r[2] for r in res]))
    got = abi.loss("approxndcg")
    _check_loss(got, want, "approxndcg max_len 5900")
    assert close(got[2], want[2])


def test_lambdaloss_workspace_form_at_max_len_3200():
    abi, parts = _one_long("lambdaloss", 3200, 32)
    c = ("ndcgLoss2PP_scheme", None, "sum", "binary")
    res = [RC.lambdaloss_expected(*p, *c) for p in parts]
    want = (sum(r[0] for r in res), np.concatenate([r[1] for r in res]), sum(r[2] for r in res), np.concatenate([r[3] for r in res]))
    got = abi.loss("lambdaloss", case=c)
    _check_loss(got, want, "lambdaloss max_len 3200")
    assert got[3] == want[2] and np.array_equal(got[4], want[3])


@pytest.mark.parametrize("scale", SCALES)
def test_python_surface_matches_the_oracle_and_derives_max_len(scale, exp):
    from allrank_amd import ragged
    e = exp[scale]
    cu, y = _t(e["cu"], torch.int32), _t(e["y"], torch.float32)
    order = _order_of(e["cu"])
    jobs = [(ragged.listNet, {}, e["listnet"]), (ragged.approxNDCGLoss, {}, e["approxndcg"])]
    for c in (("lambdaRank_scheme", None, "sum", "binary"), ("ndcgLoss2PP_scheme", 5, "mean", "natural")):
        jobs.append((ragged.lambdaLoss, dict(weighing_scheme=c[0], k=c[1], reduction=c[2], reduction_log=c[3], **RC.LAMBDA_KW),
                     e[("lambda",) + c]))
    for fn, kw, want in jobs:
        for layout in (dict(), dict(max_len=257, slate_order=order)):          # max_len derived from cu_seqlens / given
            sp = _t(e["s"], torch.float32, rg=True)
            l = fn(sp, y, cu, **dict(kw, **layout))
            l.backward()
            _check_loss((float(l.item()), sp.grad.cpu().numpy().astype(np.float64)), want, fn.__name__)
        with torch.no_grad():
            assert not fn(sp, y, cu, **kw).requires_grad
    wnd, wdc, wperm, wmr = e["metrics"]
    s = _t(e["s"], torch.float32)
    nd, perm = ragged.ndcg(s, y, cu, ats=RC.ATS, return_order=True)
    assert close(nd.cpu().numpy(), wnd) and np.array_equal(perm.cpu().numpy(), wperm)
    assert close(ragged.dcg(s, y, cu, max_len=300, slate_order=order, ats=RC.ATS).cpu().numpy(), wdc)
    assert close(ragged.mrr(s, y, cu, ats=RC.ATS).cpu().numpy(), wmr)
    # ats=None is the full slate (metrics.py:58-59): the cut-off 300 above every slate's length
    assert close(ragged.ndcg(s, y, cu).cpu().numpy()[:, 0], wnd[:, 3])
    with pytest.raises(ValueError, match="gain_function"):
        ragged.ndcg(s, y, cu, gain_function=lambda x: x)


def test_autograd_scales_the_kernel_gradient_by_the_upstream_scalar(exp):
    from allrank_amd import ragged
    e = exp[1]
    cu, y = _t(e["cu"], torch.int32), _t(e["y"], torch.float32)
    a, b = _t(e["s"], torch.float32, rg=True), _t(e["s"], torch.float32, rg=True)
    ragged.approxNDCGLoss(a, y, cu, max_len=257).backward()
    (ragged.approxNDCGLoss(b, y, cu, max_len=257) * 2.5).backward()
    assert a.grad.abs().max() > 0 and torch.equal(b.grad, a.grad * 2.5)
    abi = _Abi(e["s"], e["y"], e["cu"], 257)
    assert np.array_equal(a.grad.cpu().numpy().astype(np.float64), abi.loss("approxndcg")[1])      # the kernel's own gradient


def test_a_slate_longer_than_max_len_is_cut_to_its_first_items(exp):
    """the caller's error, but no access may leave the call's buffers: max_len 100 evaluates the slates of 255 / 256 / 257 items as
    their first 100, i.e. the batch with those slates truncated (outputs beyond the cut stay untouched)"""
    e = exp[1]
    cu = e["cu"]
    keep = np.concatenate([np.arange(cu[b], cu[b] + min(cu[b + 1] - cu[b], 100)) for b in range(len(cu) - 1)])
    cu_t = np.concatenate([[0], np.cumsum(np.minimum(np.diff(cu), 100))]).astype(np.int32)
    full, cut = _Abi(e["s"], e["y"], cu, 100), _Abi(e["s"][keep], e["y"][keep], cu_t, 100)
    for kind in ("listnet", "approxndcg"):
        a, b = full.loss(kind), cut.loss(kind)
        assert a[0] == b[0] and np.array_equal(a[1][keep], b[1]) and np.array_equal(a[2], b[2]), kind
        assert np.all(np.delete(a[1], keep) == -777), kind
    for x, y in zip(full.metrics(), cut.metrics()):
        assert np.array_equal(x[keep] if x.ndim == 1 else x, y)
