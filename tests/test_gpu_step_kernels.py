"""The optimizer and glue kernels of the explicit training step (allrank_amd/csrc/ltrx_train.hip, ltrx_extras.hip), one call at a
time through the C ABI, against the fp64 references and a-priori bars of tests/step_ref.py, -m gpu.

Every call starts from identical fp32 state and is compared on its own: |kernel - reference| <= bar for every entry, where the
bar (derived in tests/step_ref.py, shown attainable and discriminating by tests/test_step_ref_cpu.py) holds no measured number.
The index kernels, the zero pattern of relu_bwd, the row selection of posenc_fwd and the padding row of the table gradient are
compared bit for bit.  Outputs live in windows of larger buffers, 16-byte aligned: NaN around every output window, large finite
garbage around every input window (NaN around the buffer first_nonfinite scans: an over-read would be counted); both must survive,
and inputs must be unchanged.  The sizes are the smallest that reach each path: the tails, one block, and one size just above each
kernel's grid cap, where the grid-stride loop takes its second trip.  The worst error / bar of every case is logged as
parity_step_kernels.json, next to the other parity logs."""
import ctypes

import numpy as np
import pytest
import torch

from tests import step_ref as S
from tests.test_gpu_gemm_contract import EINVAL, EUNSUPPORTED, GARBAGE, Win, _libs
from tests.test_gpu_parity import DEV, _log

pytestmark = pytest.mark.gpu

F = np.float32
CASES = []


def vec(data=None, n=None, fill=np.nan):
    """a 1-D window, 4 floats into its buffer"""
    n = np.asarray(data).size if n is None else n
    return Win((1, n), n, 4, fill, None if data is None else np.asarray(data, F).reshape(1, n))


def mat(data=None, shape=None, fill=np.nan, ld=None):
    shape = np.asarray(data).shape if shape is None else shape
    return Win(shape, ld or shape[1], 4, fill, data)


class Raw(object):
    """an integer / byte array 16 bytes into a larger device buffer that is filled with a sentinel"""

    def __init__(self, data, dtype, fill):
        data = np.asarray(data, dtype).ravel()
        self.n, self.off = data.size, 16 // np.dtype(dtype).itemsize
        self.host = np.full(2 * self.off + self.n, fill, dtype)
        self.host[self.off:self.off + self.n] = data
        self.dev = torch.tensor(self.host, device=DEV)
        self.ptr = ctypes.c_void_p(self.dev.data_ptr() + 16)

    def fetch(self, what):
        now = self.dev.cpu().numpy()
        keep = np.ones(now.size, bool)
        keep[self.off:self.off + self.n] = False
        assert np.array_equal(now[keep], self.host[keep]), "%s: wrote outside the %d elements" % (what, self.n)
        return now[self.off:self.off + self.n].copy()

    def unchanged(self, what):
        assert np.array_equal(self.dev.cpu().numpy(), self.host), "%s: an input buffer was written" % what


def workspace(nbytes):
    ws = torch.zeros(int(nbytes) + 256, dtype=torch.uint8, device=DEV)
    ws[int(nbytes):] = 0xA5
    return ws, lambda what: bool((ws[int(nbytes):] == 0xA5).all()) or pytest.fail("%s: wrote past the %d workspace bytes" % (what, nbytes))


def check(kernel, case, got, ref, bar):
    r = S.worst(got, ref, bar)
    CASES.append(dict(kernel=kernel, case=str(case), worst_error_over_bar=r))
    print("%s %s: worst error / bar %.4g" % (kernel, case, r))
    assert r <= 1.0, "%s %s: worst error / bar %.4g at %d of %d entries" % (kernel, case, r, int(S.over(got, ref, bar).sum()), np.asarray(got).size)


def exact(kernel, case, ok):
    CASES.append(dict(kernel=kernel, case=str(case), worst_error_over_bar=0.0 if ok else float("inf")))
    assert ok, "%s %s: not bit-identical to the reference" % (kernel, case)


def log():
    per = {}
    for c in CASES:
        per[c["kernel"]] = max(per.get(c["kernel"], 0.0), c["worst_error_over_bar"])
    _log("step_kernels", dict(per_kernel=per, cases=CASES))


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------------------
# Adam / AdamW
# ---------------------------------------------------------------------------------------------------------------------------------
def _adam_call(n, cfg, p, g, m, v):
    LB, lib = _libs()
    P, G, M, V = vec(p), vec(g, fill=GARBAGE), vec(m), vec(v)
    step = vec([cfg["t0"]])
    gsd = vec([cfg["gsd"]], fill=GARBAGE) if cfg["gsd"] is not None else None
    LB.check(lib.ltrx_adam_step(P.ptr, G.ptr, M.ptr, V.ptr, n, cfg["lr"], cfg["b1"], cfg["b2"], cfg["eps"], cfg["wd"], cfg["decoupled"],
                                step.ptr, cfg["gs"], gsd.ptr if gsd else None, None), "adam_step")
    out = P.fetch("p")[0], M.fetch("m")[0], V.fetch("v")[0]
    assert step.fetch("step")[0, 0] == F(cfg["t0"] + 1), ("the step count is bumped by exactly 1", cfg["t0"])
    G.unchanged("grads")
    if gsd:
        gsd.unchanged("grad_scale_dev")
    return out


def _adam(n, cfg, seed):
    p, g, m, v = S.adam_inputs(np.random.default_rng(seed), n)
    kw = S.adam_args(cfg)
    got = _adam_call(n, cfg, p, g, m, v)
    tag = "n %d %s t %d b1 %.1f%s" % (n, "AdamW" if cfg["decoupled"] else "L2", kw["t"], cfg["b1"], " dev scale" if cfg["gsd"] else "")
    for name, a, r, b in zip("pmv", got, S.adam_ref(p, g, m, v, **kw), S.adam_bar(p, g, m, v, **kw)):
        check("adam_step", tag + " " + name, a, r, b)
    return (p, g, m, v), got


@pytest.mark.parametrize("n", S.ADAM_SIZES)
def test_adam_tails_options_and_step_counts(n):
    """n % 4 tails, n < 4 (empty vector loop), L2 and decoupled decay, two sets of betas / eps, the device gradient scale NULL and given,
    step counts 0 .. 99,999 before the call"""
    for k, cfg in enumerate(S.adam_configs()):
        state, got = _adam(n, cfg, 100 + 7 * n + k)
        if k % 12 == 0:
            again = _adam_call(n, cfg, *state)
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got, again)), ("not deterministic", n, cfg)
    log()


@pytest.mark.parametrize("k", [0, 1, 2])
def test_adam_second_grid_stride_trip_with_tail(k):
    _adam(S.ADAM_BIG, S.adam_big_configs()[k], 190 + k)
    log()


# ---------------------------------------------------------------------------------------------------------------------------------
# SGD
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", S.SGD_SIZES)
def test_sgd_plain_momentum_nesterov_and_scales(n):
    LB, lib = _libs()
    for k, cfg in enumerate(S.sgd_configs()):
        p, g, buf = S.sgd_inputs(np.random.default_rng(200 + k), n)
        P, G = vec(p), vec(g, fill=GARBAGE)
        Bf = vec(buf) if cfg["mom"] else None                  # momentum == 0: NULL buffer
        gsd = vec([cfg["gsd"]], fill=GARBAGE) if cfg["gsd"] is not None else None
        LB.check(lib.ltrx_sgd_step(P.ptr, G.ptr, Bf.ptr if Bf else None, n, cfg["lr"], cfg["mom"], cfg["nesterov"], cfg["wd"], cfg["gs"],
                                   gsd.ptr if gsd else None, None), "sgd_step")
        (pr, br), (pb, bb) = S.sgd_ref(p, g, buf, **cfg), S.sgd_bar(p, g, buf, **cfg)
        tag = "n %d mom %.1f nesterov %d wd %.2f%s" % (n, cfg["mom"], cfg["nesterov"], cfg["wd"], " dev scale" if gsd else "")
        check("sgd_step", tag + " p", P.fetch("p")[0], pr, pb)
        if Bf:
            check("sgd_step", tag + " buf", Bf.fetch("buf")[0], br, bb)
        G.unchanged("grads")
    log()


# ---------------------------------------------------------------------------------------------------------------------------------
# gradient clipping
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", S.CLIP_SIZES)
def test_clip_scale_and_norm(n):
    LB, lib = _libs()
    for k, (name, g, max_norm) in enumerate(S.clip_cases(np.random.default_rng(300 + n % 97), n)):
        for want_norm in (True, False):
            G, sc = vec(g, fill=GARBAGE), vec(n=1)
            no = vec(n=1) if want_norm else None
            ws, ws_ok = workspace(lib.ltrx_clip_workspace_bytes(n))
            LB.check(lib.ltrx_clip_grad_norm_scale(G.ptr, n, max_norm, sc.ptr, no.ptr if no else None, LB.ptr(ws), None), "clip")
            (sr, nr), (sb, nb) = S.clip_ref(g, max_norm), S.clip_bar(g, max_norm)
            got = sc.fetch("scale")[0, 0]
            check("clip_grad_norm_scale", "n %d %s scale" % (n, name), got, sr, sb)
            if name == "below":
                assert got == F(1.0)
            if no:
                check("clip_grad_norm_scale", "n %d %s norm" % (n, name), no.fetch("norm")[0, 0], nr, nb)
            ws_ok("clip")
            G.unchanged("grads")
    log()


# ---------------------------------------------------------------------------------------------------------------------------------
# column sums
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,ld", S.COLSUM_SHAPES)
def test_colsum_strided_and_accumulating(M, N, ld):
    LB, lib = _libs()
    a, old = S.colsum_inputs(np.random.default_rng(400 + M % 97), M, N)
    A = mat(a, fill=GARBAGE, ld=ld)
    for acc in (0, 1):
        out = vec(old) if acc else vec(n=N)
        ws, ws_ok = workspace(lib.ltrx_colsum_workspace_bytes(M, N))
        LB.check(lib.ltrx_colsum(A.ptr, M, N, ld, out.ptr, acc, LB.ptr(ws), None), "colsum")
        check("colsum", "%dx%d ld %d accumulate %d" % (M, N, ld, acc), out.fetch("out")[0], S.colsum_ref(a, old, acc), S.colsum_bar(a, old, acc))
        ws_ok("colsum")
    A.unchanged("a")
    log()


# ---------------------------------------------------------------------------------------------------------------------------------
# ReLU backward
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", S.RELU_SIZES)
def test_relu_bwd_zero_pattern_is_exact(n):
    LB, lib = _libs()
    dr, r = S.relu_inputs(np.random.default_rng(500 + n % 97), n)
    D, Rw = vec(dr), vec(r, fill=GARBAGE)
    LB.check(lib.ltrx_relu_bwd(D.ptr, Rw.ptr, n, 1.25, None), "relu_bwd")
    got, ref = D.fetch("dr")[0], S.relu_bwd_ref(dr, r, 1.25)
    check("relu_bwd", "n %d" % n, got, ref, S.relu_bwd_bar(dr, r, 1.25))
    dead = ~(r > 0)                                             # 0, -0.0 and the negatives (dr is NaN there); the positive denormal is alive
    exact("relu_bwd", "n %d zero pattern" % n, not bits(got[dead]).any() and bool((got[~dead] != 0).all()))
    Rw.unchanged("r")
    log()


# ---------------------------------------------------------------------------------------------------------------------------------
# first non-finite segment
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", S.NONFINITE_SIZES)
def test_first_nonfinite_segment_and_count(n):
    LB, lib = _libs()
    seg = S.nonfinite_segments(n)
    base = S.nonfinite_base(np.random.default_rng(600 + n % 97), n)
    segs = Raw(seg, np.int64, 2 ** 62)
    for place in S.nonfinite_placements(n, seg):
        for bad in (np.nan, np.inf, -np.inf):
            buf = base.copy()
            buf[place] = bad
            B, out = vec(buf, fill=np.nan), Raw([-7, -7], np.int32, -7)
            LB.check(lib.ltrx_first_nonfinite(B.ptr, n, segs.ptr, len(seg), out.ptr, None), "first_nonfinite")
            got = tuple(int(x) for x in out.fetch("out"))
            exact("first_nonfinite", "n %d at %s %r" % (n, place, bad), got == S.first_nonfinite_ref(buf, seg))
            B.unchanged("buf")
    segs.unchanged("seg_start")
    log()


# ---------------------------------------------------------------------------------------------------------------------------------
# packed row index
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(S.PACKED_LENGTHS)))
def test_packed_row_index_with_empty_slates(k):
    LB, lib = _libs()
    lens = S.PACKED_LENGTHS[k]
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    B, L, n = len(lens), max(max(lens), 1) + 3, int(cu[-1])
    cus, idx = Raw(cu, np.int32, 10 ** 9), Raw(np.full(max(n, 4), -7), np.int32, -7)
    LB.check(lib.ltrx_packed_row_index(cus.ptr, B, L, n, idx.ptr, None), "packed_row_index")
    got = idx.fetch("idx")
    exact("packed_row_index", "lengths %s" % lens, np.array_equal(got[:n], S.packed_row_index_ref(cu, L)) and bool((got[n:] == -7).all()))
    cus.unchanged("cu_seqlens")
    log()


# ---------------------------------------------------------------------------------------------------------------------------------
# nn.LayerNorm forward and its parameter gradients
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,D", S.LN_SHAPES)
def test_layernorm_torch_fwd_and_parameter_gradients(rows, D):
    """row 1 constant, row 2 with |mean| / std of 1e4 (its bar carries the mean's rounding); dw / db from ltrx_layernorm_bwd called
    with the statistics the forward saved (D >= 2: that entry point refuses D == 1 before it launches)"""
    LB, lib = _libs()
    x, wt, b, gy = S.ln_inputs(np.random.default_rng(700 + rows % 97), rows, D)
    X, Wt, Bs = mat(x, fill=GARBAGE), vec(wt, fill=GARBAGE), vec(b, fill=GARBAGE)
    Y, Mn, Rs = mat(shape=(rows, D)), vec(n=rows), vec(n=rows)
    LB.check(lib.ltrx_layernorm_torch_fwd(X.ptr, Wt.ptr, Bs.ptr, rows, D, 1e-5, Y.ptr, Mn.ptr, Rs.ptr, None), "layernorm_torch_fwd")
    mean, rstd = Mn.fetch("mean")[0], Rs.fetch("rstd")[0]
    Mn.host, Rs.host = Mn.dev.cpu().numpy().copy(), Rs.dev.cpu().numpy().copy()     # from here on inputs: the device's own statistics
    tag = "%dx%d" % (rows, D)
    for name, a, r, bb in zip(("y", "mean", "rstd"), (Y.fetch("y"), mean, rstd), S.ln_ref(x, wt, b, 1e-5), S.ln_bar(x, wt, b, 1e-5)):
        check("layernorm_torch_fwd", tag + " " + name, a, r, bb)
    Gy, Dx, Da, Db = mat(gy, fill=GARBAGE), mat(shape=(rows, D)), vec(n=D), vec(n=D)
    ws, ws_ok = workspace(lib.ltrx_layernorm_bwd_workspace_bytes(rows, D))
    rc = lib.ltrx_layernorm_bwd(Gy.ptr, X.ptr, Wt.ptr, Mn.ptr, Rs.ptr, None, rows, D, 1e-5, Dx.ptr, Da.ptr, Db.ptr, LB.ptr(ws), None)
    if D < 2:
        assert rc == EINVAL and np.isnan(Da.fetch("da")).all() and np.isnan(Db.fetch("db")).all()
    else:
        LB.check(rc, "layernorm_bwd")
        (dwr, dbr), (dwb, dbb) = S.ln_grad_ref(x, mean, rstd, wt, gy), S.ln_grad_bar(x, mean, rstd, gy)
        check("layernorm_bwd (nn.LayerNorm statistics)", tag + " dw", Da.fetch("da")[0], dwr, dwb)
        check("layernorm_bwd (nn.LayerNorm statistics)", tag + " db", Db.fetch("db")[0], dbr, dbb)
        Dx.fetch("dx")
        ws_ok("layernorm_bwd")
    for wnd in (X, Wt, Bs, Gy, Mn, Rs):
        wnd.unchanged(tag)
    log()


# ---------------------------------------------------------------------------------------------------------------------------------
# positional encoding
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,D,pad", S.POSENC_SHAPES)
def test_posenc_forward_and_table_gradient(M, D, pad):
    LB, lib = _libs()
    x, table, idx, mask, dx = S.posenc_inputs(np.random.default_rng(800 + M % 97), M, D, pad)
    X, Z, T, DX = mat(x, fill=GARBAGE), mat(np.zeros_like(x), fill=GARBAGE), mat(table, fill=GARBAGE), mat(dx, fill=GARBAGE)
    I, Mk = Raw(idx, np.int64, 1), Raw(mask, np.uint8, 0)
    for name, mk, mptr in (("no mask", None, None), ("mask", mask, Mk.ptr)):
        tag = "%dx%d pad %d %s" % (M, D, pad, name)
        Y = mat(shape=(M, D))
        LB.check(lib.ltrx_posenc_fwd(X.ptr, T.ptr, I.ptr, mptr, M, D, pad, 8.0, Y.ptr, None), "posenc_fwd")
        check("posenc_fwd", tag, Y.fetch("y"), S.posenc_ref(x, table, idx, mk, pad, 8.0), S.posenc_bar(x, table, idx, mk, pad, 8.0))
        Y0 = mat(shape=(M, D))                                 # x = 0: y is the selected table row, bit for bit
        LB.check(lib.ltrx_posenc_fwd(Z.ptr, T.ptr, I.ptr, mptr, M, D, pad, 8.0, Y0.ptr, None), "posenc_fwd")
        exact("posenc_fwd", tag + " row selection", np.array_equal(bits(Y0.fetch("y")), bits(table[S.posenc_rows(idx, mk, pad)])))
        runs = []
        for _ in range(2):
            DT = mat(shape=(pad + 1, D))
            LB.check(lib.ltrx_posenc_table_bwd(DX.ptr, I.ptr, mptr, M, D, pad, DT.ptr, None), "posenc_table_bwd")
            runs.append(DT.fetch("dtable"))
        check("posenc_table_bwd", tag, runs[0], S.posenc_table_bwd_ref(dx, idx, mk, pad), S.posenc_table_bwd_bar(dx, idx, mk, pad))
        exact("posenc_table_bwd", tag + " padding row, repeat", not bits(runs[0][pad]).any() and np.array_equal(bits(runs[0]), bits(runs[1])))
    for wnd in (X, Z, T, DX, I, Mk):
        wnd.unchanged("posenc")
    log()


# ---------------------------------------------------------------------------------------------------------------------------------
# scale_inplace and the output activations
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 1048576 + 3])
def test_scale_inplace(n):
    LB, lib = _libs()
    x = S.spread(np.random.default_rng(900 + n % 97), n, -20, 20)
    X = vec(x)
    LB.check(lib.ltrx_scale_inplace(X.ptr, n, 11.313708, None), "scale_inplace")
    check("scale_inplace", "n %d" % n, X.fetch("x")[0], S.scale_ref(x, 11.313708), S.scale_bar(x, 11.313708))
    log()


@pytest.mark.parametrize("kind", [1, 2])
def test_output_activation_forward_and_backward_at_saturation(kind):
    LB, lib = _libs()
    z, dy = S.out_act_inputs(np.random.default_rng(950))
    n = z.size
    Z, Y, DY, DZ = vec(z, fill=GARBAGE), vec(n=n), vec(dy, fill=GARBAGE), vec(n=n)
    LB.check(lib.ltrx_out_act_fwd(Z.ptr, n, kind, Y.ptr, None), "out_act_fwd")
    y = Y.fetch("y")[0]
    check("out_act_fwd", "kind %d" % kind, y, S.out_act_ref(z, kind), S.out_act_bar(z, kind))
    Y.host = Y.dev.cpu().numpy().copy()                         # from here on y is an input: the device's own
    LB.check(lib.ltrx_out_act_bwd(DY.ptr, Y.ptr, n, kind, DZ.ptr, None), "out_act_bwd")
    check("out_act_bwd", "kind %d" % kind, DZ.fetch("dz")[0], S.out_act_bwd_ref(dy, y, kind), S.out_act_bwd_bar(dy, y, kind))
    for wnd in (Z, Y, DY):
        wnd.unchanged("out_act")
    log()


# ---------------------------------------------------------------------------------------------------------------------------------
# the argument contract: only what the wrappers refuse before they launch anything
# ---------------------------------------------------------------------------------------------------------------------------------
def test_argument_contract_refuses_before_launching():
    LB, lib = _libs()
    buf = vec(np.ones(64, F))                                   # every non-NULL pointer below; must come through untouched
    p, q = buf.ptr, ctypes.c_void_p(buf.ptr.value + 4)          # q: 4 bytes off 16-byte alignment
    calls = {
        "adam": lambda a: lib.ltrx_adam_step(a.get("p", p), a.get("g", p), a.get("m", p), a.get("v", p), a.get("n", 8), 1e-3, 0.9, 0.999, 1e-8, 0.0, 0,
                                             a.get("step", p), 1.0, None, None),
        "sgd": lambda a: lib.ltrx_sgd_step(a.get("p", p), a.get("g", p), a.get("buf", p), a.get("n", 8), 0.1, a.get("mom", 0.9), a.get("nesterov", 0),
                                           0.0, 1.0, None, None),
        "clip": lambda a: lib.ltrx_clip_grad_norm_scale(a.get("g", p), a.get("n", 8), a.get("max_norm", 1.0), a.get("out", p), None, a.get("ws", p), None),
        "colsum": lambda a: lib.ltrx_colsum(a.get("a", p), a.get("M", 2), a.get("N", 4), a.get("ld", 4), a.get("out", p), 0, a.get("ws", p), None),
        "relu": lambda a: lib.ltrx_relu_bwd(a.get("dr", p), a.get("r", p), a.get("n", 8), 1.0, None),
        "nonfinite": lambda a: lib.ltrx_first_nonfinite(a.get("buf", p), a.get("n", 8), a.get("seg", p), a.get("n_seg", 1), a.get("out", p), None),
        "packed": lambda a: lib.ltrx_packed_row_index(a.get("cu", p), a.get("B", 2), a.get("L", 4), a.get("n", 4), a.get("idx", p), None),
        "ln": lambda a: lib.ltrx_layernorm_torch_fwd(a.get("x", p), a.get("w", p), a.get("b", p), a.get("rows", 2), a.get("D", 4), 1e-5, a.get("y", p),
                                                     a.get("mean", p), a.get("rstd", p), None),
        "pe": lambda a: lib.ltrx_posenc_fwd(a.get("x", p), a.get("table", p), a.get("idx", p), None, a.get("M", 2), a.get("D", 4), a.get("pad", 1), 1.0,
                                            a.get("y", p), None),
        "pe_bwd": lambda a: lib.ltrx_posenc_table_bwd(a.get("dx", p), a.get("idx", p), None, a.get("M", 2), a.get("D", 4), a.get("pad", 1), a.get("dt", p), None),
        "scale": lambda a: lib.ltrx_scale_inplace(a.get("x", p), a.get("n", 8), 2.0, None),
        "act": lambda a: lib.ltrx_out_act_fwd(a.get("z", p), a.get("n", 8), a.get("kind", 1), a.get("y", p), None),
        "act_bwd": lambda a: lib.ltrx_out_act_bwd(a.get("dy", p), a.get("y", p), a.get("n", 8), a.get("kind", 1), a.get("dz", p), None),
    }
    refused = [("adam", k, None) for k in ("p", "g", "m", "v", "step")] + [("adam", "n", 0)]
    refused += [("sgd", "p", None), ("sgd", "g", None), ("sgd", "buf", None), ("sgd", "n", 0)]
    refused += [("clip", "g", None), ("clip", "out", None), ("clip", "ws", None), ("clip", "n", 0), ("clip", "max_norm", 0.0), ("clip", "max_norm", -1.0)]
    refused += [("colsum", "a", None), ("colsum", "out", None), ("colsum", "ws", None), ("colsum", "M", 0), ("colsum", "N", 0), ("colsum", "ld", 3)]
    refused += [("relu", "dr", None), ("relu", "r", None), ("relu", "n", 0), ("relu", "n", 6)]
    refused += [("nonfinite", "buf", None), ("nonfinite", "seg", None), ("nonfinite", "out", None), ("nonfinite", "n", 0), ("nonfinite", "n_seg", 0),
                ("nonfinite", "buf", q)]
    refused += [("packed", "cu", None), ("packed", "idx", None), ("packed", "B", 0), ("packed", "L", 0), ("packed", "n", -1), ("packed", "n", 9)]
    refused += [("ln", k, None) for k in ("x", "w", "b", "y", "mean", "rstd")] + [("ln", "rows", 0), ("ln", "D", 0)]
    refused += [("pe", k, None) for k in ("x", "table", "idx", "y")] + [("pe", "M", 0), ("pe", "D", 0), ("pe", "pad", -1)]
    refused += [("pe_bwd", k, None) for k in ("dx", "idx", "dt")] + [("pe_bwd", "M", 0), ("pe_bwd", "D", 0), ("pe_bwd", "pad", -1)]
    refused += [("scale", "x", None), ("act", "z", None), ("act", "y", None), ("act", "kind", 0), ("act", "kind", 3)]
    refused += [("act_bwd", k, None) for k in ("dy", "y", "dz")] + [("act_bwd", "kind", 0), ("act_bwd", "kind", 3)]
    for (fn, key, val) in refused:
        assert calls[fn]({key: val}) == EINVAL, (fn, key, val)
    assert calls["sgd"](dict(mom=0.0, nesterov=1)) == EINVAL                      # Nesterov without momentum
    for args in (dict(D=6), dict(x=q), dict(table=q), dict(y=q)):                  # posenc_fwd moves 16 bytes at a time
        assert calls["pe"](args) == EUNSUPPORTED, args
    assert calls["pe_bwd"](dict(D=4097)) == EUNSUPPORTED                           # 4 D floats of LDS
    for fn in ("packed", "scale", "act", "act_bwd"):                               # nothing to do: success, nothing written
        assert calls[fn](dict(n=0)) == 0, fn
    torch.cuda.synchronize()
    buf.unchanged("a refused call")
