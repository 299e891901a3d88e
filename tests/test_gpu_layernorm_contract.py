"""The contract of every arm of the custom LayerNorm kernels (allrank_amd/csrc/ltrx_layernorm.hip, ltrx_rowreg.h), -m gpu.

One call through the C ABI per comparison, and one assertion for EVERY entry of every output -- xsum, mean, rstd, y, dx, the partial
rows [da | db], da and db (summed by ltrx_layernorm_bwd's own reduce kernel and by ltrx_reduce_group):  |kernel - fp64 reference| <=
bar, with the references, the derivation of the entrywise bars, the defect models and the case table in tests/layernorm_ref.py.
tests/test_layernorm_ref_cpu.py is the evidence that the bars bite: an fp32 transcription in the kernels' operation order stays inside
them on every case, every defect model (biased variance, eps inside the square root, a padded mean, a dropped tail, a residual added
late, a scaled x; no gm, D for D - 1, a wrong sign, no dres, da on dy a, a missing row, a misattributed partial row) is outside.

The table reaches every instantiation: the scalar kernels (D = 2 .. 2048, and D = 512 with x / dy or y / dx 4 bytes off 16-byte
alignment, on the data of the aligned 37 x 512 case: both arms meet the contract on the same rows), ltrx_layernorm_fwd_vec_kernel<1..4>,
ltrx_layernorm_bwd_vec_kernel<1..4, 4> and <1..2, 16>, each above and below its grid cap, and every (rows, D) and launch shape of
tests/test_gpu_norm_head.py and tests/test_gpu_tn_group_ln.py: those compare the fused norm + head and the weight-gradient side job bit
for bit with the kernels held to fp64 here, so the contract carries over to them.

Around every window the buffers hold sentinels (NaN around outputs, 3e37 around inputs, 0xA5 behind a workspace of exactly
ltrx_layernorm_bwd_workspace_bytes, NaN inside it) that must survive; inputs must be unchanged; a second identical call gives the same
bits; *partial_rows_out is the restated grid.  The backward is handed the mean and rstd the forward kernel wrote.  The worst error / bar
of every (kernel, case, output) is logged as parity_layernorm_contract.json."""
import ctypes

import numpy as np
import pytest
import torch

from tests import layernorm_ref as R
from tests.test_gpu_gemm_contract import EINVAL, EUNSUPPORTED, GARBAGE, Win
from tests.test_gpu_parity import DEV, _log
from tests.test_gpu_step_kernels import Raw

pytestmark = pytest.mark.gpu

F = np.float32
TAIL = 4096
ROWS = {}


def _libs():
    from allrank_amd import _lib as LB
    return LB, LB.lib()


def _in(data, off=4):
    data = np.atleast_2d(np.asarray(data, F))
    return Win(data.shape, data.shape[1], off, GARBAGE, data)


def _out(rows, cols, off=4):
    return Win((rows, cols), cols, off, np.nan)


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _run(what, fn):
    """a library call; after a device error nothing more is launched"""
    LB, _ = _libs()
    try:
        LB.check(fn(), what)
        torch.cuda.synchronize()
    except RuntimeError as e:
        if "hip" in str(e).lower():
            pytest.exit("%s: %s -- nothing more is launched on a device that reported an error" % (what, e), returncode=3)
        raise


def _check(kernel, c, opt, output, got, ref, bar):
    r = R.worst(got, ref, bar)
    key = (kernel, c.name, output)
    ROWS[key] = max(ROWS.get(key, 0.0), r)
    print("%s, %s, %s: %s worst error / bar %.4g" % (kernel, c.name, opt.name, output, r))
    assert r <= 1.0, "%s, %s, %s: %s is outside its bar at %d of %d entries, worst error / bar %.4g" % (
        kernel, c.name, opt.name, output, int(R.over(got, ref, bar).sum()), np.asarray(got).size, r)


def _log_rows():
    _log("layernorm_contract", [dict(kernel=k[0], case=k[1], output=k[2], worst_error_over_bar=v) for k, v in sorted(ROWS.items())])


class Problem(object):
    """one case on the device: its input windows, and the call + check of one forward or backward option"""

    def __init__(self, c):
        self.c, self.X, self.vec = c, R.inputs(c), R.is_vec(c)
        X = self.X
        off_in = 5 if c.misaligned == "in" else 4
        self.off_out = 5 if c.misaligned == "out" else 4
        self.x, self.dy = _in(X["x"], off_in), _in(X["dy"], off_in)
        self.res, self.dres, self.a, self.b = _in(X["res"]), _in(X["dres"]), _in(X["a"]), _in(X["b"])
        self.step = Raw([R.WORD], np.int32, 0x5A5A5A5A)
        self.stats = None

    def _arm(self, *wins):
        """the windows give the arm predicate the answer the case is meant for"""
        ok = R.ln_vec_ok(self.c.D, [w.ptr.value for w in wins if w is not None])
        assert ok == self.vec, "%s: the pointers' alignment selects another arm than the table says" % self.c.name

    # ---- forward
    def fwd_call(self, opt):
        _, lib = _libs()
        c = self.c
        xs = _out(c.rows, c.D) if opt.xsum else None
        y, mean, rstd = _out(c.rows, c.D, self.off_out), _out(1, c.rows), _out(1, c.rows)
        res = self.res if opt.res else None
        self._arm(self.x, y, res, self.a, self.b, xs)
        what = "%s, %s: ltrx_layernorm_fwd" % (c.name, opt.name)
        _run(what, lambda: lib.ltrx_layernorm_fwd(self.x.ptr, res.ptr if res else None, self.a.ptr, self.b.ptr, c.rows, c.D, c.eps,
                                                   xs.ptr if xs else None, y.ptr, mean.ptr, rstd.ptr, opt.p, R.SEED,
                                                   self.step.ptr if opt.word is not None else None, None))
        return dict(xsum=xs.fetch(what + " xsum") if xs else None, y=y.fetch(what + " y"), mean=mean.fetch(what + " mean")[0],
                    rstd=rstd.fetch(what + " rstd")[0])

    def fwd(self, opt, again=False):
        c, X = self.c, self.X
        kernel = R.fwd_kernel(c.D, self.vec)
        got = self.fwd_call(opt)
        res = X["res"] if opt.res else None
        scale = R.keep_scale(opt.p, R.SEED, opt.word, c.rows, c.D) if opt.res else None
        v = X["x"]
        if opt.xsum:                                       # first, on its own; the rest is referred to the xsum the kernel wrote
            v = got["xsum"]
            _check(kernel, c, opt, "xsum", v, R.xsum_ref(X["x"], res, scale), R.xsum_bar(X["x"], res, scale))
            if scale is not None and scale.size >= 4096:
                assert 0.27 < (scale == 0).mean() < 0.33, "the keep mask is not p = 0.3's"
        ref = dict(zip(("mean", "rstd", "y"), R.fwd_ref(v, X["a"], X["b"], c.eps)))
        bar = dict(zip(("mean", "rstd", "y"), R.fwd_bar(v, X["a"], X["b"], c.eps, self.vec)))
        for t in ("mean", "rstd", "y"):
            _check(kernel, c, opt, t, got[t], ref[t], bar[t])
        if again:
            twice = self.fwd_call(opt)
            assert all(twice[t] is None if got[t] is None else np.array_equal(_bits(got[t]), _bits(twice[t])) for t in got), \
                "%s, %s: a second forward gives other bits" % (c.name, opt.name)
        if not opt.res:
            self.stats = (got["mean"], got["rstd"])
        return got

    # ---- backward
    def bwd_call(self, opt, mean, rstd):
        _, lib = _libs()
        c = self.c
        dx, da, db = _out(c.rows, c.D, self.off_out), _out(1, c.D), _out(1, c.D)
        dres = self.dres if opt.dres else None
        nws = lib.ltrx_layernorm_bwd_workspace_bytes(c.rows, c.D)
        assert nws == R.workspace_bytes(c.rows, c.D)
        ws = torch.full((nws + TAIL,), 0xFF, dtype=torch.uint8, device=DEV)          # NaN inside: an unwritten partial entry shows
        ws[nws:] = 0xA5
        wsp = ctypes.c_void_p(ws.data_ptr())
        self._arm(self.dy, self.x, dx, self.a, dres)
        assert ws.data_ptr() % 16 == 0
        grid, wpb = R.ln_bwd_shape(c.rows, c.D, self.vec)
        what = "%s, %s: ltrx_layernorm_%s" % (c.name, opt.name, opt.entry)
        args = (self.dy.ptr, self.x.ptr, self.a.ptr, mean.ptr, rstd.ptr, dres.ptr if dres else None, c.rows, c.D, c.eps, dx.ptr)
        out = {}
        if opt.entry == "bwd":
            _run(what, lambda: lib.ltrx_layernorm_bwd(*args, da.ptr, db.ptr, wsp, None))
        else:
            pr = ctypes.c_int(-7)
            _run(what, lambda: lib.ltrx_layernorm_bwd_partial(*args, wsp, ctypes.byref(pr), None))
            assert pr.value == grid, "%s: %d partial rows, the launch shape has %d" % (what, pr.value, grid)
            out["partial"] = ws[:grid * 2 * c.D * 4].view(torch.float32).cpu().numpy().reshape(grid, 2, c.D).copy()
            vp, n = ctypes.c_void_p * 2, 2
            _run(what + " + ltrx_reduce_group", lambda: lib.ltrx_reduce_group(
                n, vp(ws.data_ptr(), ws.data_ptr() + 4 * c.D), (ctypes.c_int * n)(grid, grid), (ctypes.c_size_t * n)(2 * c.D, 2 * c.D),
                (ctypes.c_size_t * n)(c.D, c.D), vp(da.ptr.value, db.ptr.value), None))
            assert np.array_equal(_bits(ws[:grid * 2 * c.D * 4].view(torch.float32).cpu().numpy()), _bits(out["partial"]).ravel()), what
        assert bool((ws[nws:] == 0xA5).all()), "%s: wrote behind its %d-byte workspace" % (what, nws)
        assert grid * 2 * c.D * 4 <= nws
        out.update(dx=dx.fetch(what + " dx"), da=da.fetch(what + " da")[0], db=db.fetch(what + " db")[0])
        return out

    def bwd(self, opt, again=False):
        c, X = self.c, self.X
        _statistics(self)
        m, r = self.stats
        mean, rstd = _in(m), _in(r)
        kernel = R.bwd_kernel(c.rows, c.D, self.vec)
        shape = R.ln_bwd_shape(c.rows, c.D, self.vec)
        got = self.bwd_call(opt, mean, rstd)
        args = (X["dy"], X["x"], X["a"], m, r, X["dres"] if opt.dres else None, c.eps)
        ref, bar = R.bwd_ref(*args, shape=shape), R.bwd_bar(*args, self.vec, shape)
        _check(kernel, c, opt, "dx", got["dx"], ref["dx"], bar["dx"])
        if c.rows - 1 > R.ZERO_DY_ROW and not opt.dres:
            assert not got["dx"][R.ZERO_DY_ROW].any(), "%s: a row without dy has a gradient" % c.name
        tag = "" if opt.entry == "bwd" else "_group"
        if opt.entry == "partial":
            _check(kernel, c, opt, "partial rows", got["partial"], ref["partial"], bar["partial"])
        _check(kernel, c, opt, "da" + tag, got["da"], ref["da"], bar["da" + tag])
        _check(kernel, c, opt, "db" + tag, got["db"], ref["db"], bar["db" + tag])
        if again:
            twice = self.bwd_call(opt, mean, rstd)
            assert all(np.array_equal(_bits(got[t]), _bits(twice[t])) for t in got), "%s, %s: a second backward gives other bits" % (c.name, opt.name)
        mean.unchanged(c.name + " mean")
        rstd.unchanged(c.name + " rstd")

    def inputs_unchanged(self):
        for name in ("x", "dy", "res", "dres", "a", "b", "step"):
            getattr(self, name).unchanged("%s %s" % (self.c.name, name))


def _statistics(pr):
    """the mean and rstd the backward is handed: the forward kernel's own, of x alone"""
    if pr.stats is None:
        got = pr.fwd_call(R.FWD_OPTIONS[0])
        pr.stats = (got["mean"], got["rstd"])


SMALL = [c for c in R.CASES if c.rows * c.D < R.LARGE]
BIG = [c for c in R.CASES if c.rows * c.D >= R.LARGE]


@pytest.mark.parametrize("c", [pytest.param(c, id=c.name) for c in SMALL])
def test_layernorm_arm_meets_the_entrywise_contract(c):
    pr = Problem(c)
    for k, opt in enumerate(R.fwd_options(c)):
        pr.fwd(opt, again=k == len(R.fwd_options(c)) - 1)
    _statistics(pr)
    for k, opt in enumerate(R.bwd_options(c)):
        pr.bwd(opt, again=k in (0, len(R.bwd_options(c)) - 1))
    pr.inputs_unchanged()
    _log_rows()


@pytest.mark.parametrize("c,k", [pytest.param(c, k, id="%s, %s" % (c.name, R.fwd_options(c)[k].name)) for c in BIG for k in range(len(R.fwd_options(c)))])
def test_layernorm_forward_at_the_grid_caps_and_the_wide_shapes(c, k):
    pr = Problem(c)
    pr.fwd(R.fwd_options(c)[k], again=k == 1)
    pr.inputs_unchanged()
    _log_rows()


@pytest.mark.parametrize("c,k", [pytest.param(c, k, id="%s, %s" % (c.name, R.bwd_options(c)[k].name)) for c in BIG for k in range(len(R.bwd_options(c)))])
def test_layernorm_backward_at_the_grid_caps_and_the_wide_shapes(c, k):
    pr = Problem(c)
    _statistics(pr)
    pr.bwd(R.bwd_options(c)[k], again=True)
    pr.inputs_unchanged()
    _log_rows()


def test_the_comparison_tells_a_biased_variance_and_one_missing_row_among_the_wide_shapes():
    """negative controls on the device's own outputs at the flagship shape (sixteen waves): the rstd that meets the contract is outside
    the bar around the biased-variance value on every row with a spread, and the da / db that meet it are outside the bars around the sums
    without the last row -- 6e-5 of a column sum against a chain bar of 3e-6 of it -- on most columns (dy spans nine binades)"""
    c = [c for c in R.CASES if (c.rows, c.D) == (R.WIDE_ROWS + 5, 512)][0]
    pr = Problem(c)
    _statistics(pr)
    X, (m, r) = pr.X, pr.stats
    _, r64, _ = R.fwd_ref(X["x"], X["a"], X["b"], c.eps)
    bar = R.fwd_bar(X["x"], X["a"], X["b"], c.eps, pr.vec)[1]
    biased = 1.0 / ((1.0 / r64 - R.w(c.eps)) * np.sqrt((c.D - 1.0) / c.D) + R.w(c.eps))
    assert not R.over(r, r64, bar).any()
    live = np.arange(c.rows) != R.CONST_ROW
    assert R.over(r, biased, bar)[live].all() and not R.over(r, biased, bar)[R.CONST_ROW]
    opt = R.BWD_OPTIONS[1]
    got = pr.bwd_call(opt, _in(m), _in(r))
    shape = R.ln_bwd_shape(c.rows, c.D, pr.vec)
    assert shape == (R.LN_BWD_G16, 16)
    args = (X["dy"], X["x"], X["a"], m, r, None, c.eps)
    ref, bars = R.bwd_ref(*args), R.bwd_bar(*args, pr.vec, shape)
    last_b = R.f64(X["dy"][-1])
    last_a = last_b * (R.f64(X["x"][-1]) - float(m[-1])) * float(r[-1])
    assert not R.over(got["da"], ref["da"], bars["da"]).any() and not R.over(got["db"], ref["db"], bars["db"]).any()
    assert R.over(got["da"], ref["da"] - last_a, bars["da"]).mean() > 0.5 and R.over(got["db"], ref["db"] - last_b, bars["db"]).mean() > 0.5


def test_refusals_return_without_writing():
    _, lib = _libs()
    rows, D, eps = 8, 256, 1e-6
    rng = np.random.default_rng(5)
    x, res, dy, dres = (_in(rng.standard_normal((rows, D))) for _ in range(4))
    a, b, mean, rstd = _in(np.ones(D)), _in(np.zeros(D)), _in(np.zeros(rows)), _in(np.ones(rows))
    big = _in(np.ones((2, 2049)))
    outs = dict(xs=_out(rows, D), y=_out(rows, D), m=_out(1, rows), r=_out(1, rows), dx=_out(rows, D), da=_out(1, D), db=_out(1, D), wide=_out(2, 2049))
    ws = torch.zeros(lib.ltrx_layernorm_bwd_workspace_bytes(2, 2049) + TAIL, dtype=torch.uint8, device=DEV)
    wsp = ctypes.c_void_p(ws.data_ptr())
    pr = ctypes.c_int(-7)
    P = lambda w: w.ptr if w is not None else None      # noqa: E731

    def fwd(x=x, res=None, a=a, b=b, rows=rows, D=D, xs=outs["xs"], y=outs["y"], m=outs["m"], r=outs["r"], p=0.0):
        return lib.ltrx_layernorm_fwd(P(x), P(res), P(a), P(b), rows, D, eps, P(xs), P(y), P(m), P(r), p, R.SEED, None, None)

    def bwd(dy=dy, x=x, a=a, mean=mean, rstd=rstd, rows=rows, D=D, dx=outs["dx"], da=outs["da"], db=outs["db"], ws=wsp, partial=False, pr=pr):
        head = (P(dy), P(x), P(a), P(mean), P(rstd), P(dres), rows, D, eps, P(dx))
        if partial:
            return lib.ltrx_layernorm_bwd_partial(*head, ws, ctypes.byref(pr) if pr is not None else None, None)
        return lib.ltrx_layernorm_bwd(*head, P(da), P(db), ws, None)

    for kw in (dict(x=None), dict(a=None), dict(b=None), dict(y=None), dict(m=None), dict(r=None), dict(rows=0), dict(rows=-3), dict(D=1),
               dict(D=0), dict(res=res, xs=None), dict(res=res, p=-0.1), dict(res=res, p=1.0), dict(res=res, p=float("nan")), dict(p=1.0)):
        assert fwd(**kw) == EINVAL, ("forward", sorted(kw))
    for partial in (False, True):
        for kw in (dict(dy=None), dict(x=None), dict(a=None), dict(mean=None), dict(rstd=None), dict(dx=None), dict(ws=None), dict(rows=0),
                   dict(rows=-3), dict(D=1)):
            assert bwd(partial=partial, **kw) == EINVAL, ("backward", partial, sorted(kw))
        assert bwd(partial=partial, dy=big, x=big, a=big, rows=2, D=2049, dx=outs["wide"]) == EUNSUPPORTED
    assert bwd(da=None) == EINVAL and bwd(db=None) == EINVAL and bwd(partial=True, pr=None) == EINVAL
    assert lib.ltrx_layernorm_bwd_workspace_bytes(0, D) == 0 and lib.ltrx_layernorm_bwd_workspace_bytes(rows, 0) == 0
    torch.cuda.synchronize()
    for name, wnd in outs.items():
        wnd.unchanged("a refused call wrote " + name)
    for wnd in (x, res, dy, dres, a, b, mean, rstd, big):
        wnd.unchanged("a refused call wrote an input")
    assert pr.value == -7 and not bool(ws.any()), "a refused backward wrote its workspace or the partial row count"
    # the largest width the backward accepts does run (64 KiB of dynamic LDS): tests/layernorm_ref.py's D = 2048 cases
    assert fwd(D=2049, rows=2, x=big, a=big, b=big, xs=None, y=outs["wide"]) == 0
    torch.cuda.synchronize()
    assert np.isfinite(outs["wide"].fetch("y at D = 2049")).all()
