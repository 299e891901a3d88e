"""fp64 references, a-priori entrywise bars, fp32 transcriptions and the case table of the custom LayerNorm kernels
(allrank_amd/csrc/ltrx_layernorm.hip, ltrx_rowreg.h)  --  TEST INFRASTRUCTURE, plain numpy, needs no GPU.

As in tests/step_ref.py there are, for the forward and for the backward, functions that take the fp32 operands exactly as the
kernel receives them:

    *_ref   the operation in fp64 through oracle/model_oracle.py (custom_ln_fwd / custom_ln_bwd), eps the fp32 value widened
    *_bar   the bound on |kernel - *_ref| per entry: (fp32 roundings on the longest path) * u * (sum of |terms|) plus the
            propagated error of whatever the entry depends on; gam(k) = k u / (1 - k u), u = 2^-24.  No measured number.
    *_f32   the kernels' arithmetic in np.float32 in the operation order of the source, with ``wrong=`` one-line defects
            (tests/test_layernorm_ref_cpu.py: the transcription is inside every bar, every applicable defect outside)

The two arms.  `vec` (ln_vec_ok: D % 256 == 0, D <= 1024, every pointer 16-byte aligned): lane l holds the float4 columns
4 (l + 64 t), t < NV = D / 256; else the scalar kernels: lane l walks columns l, l + 64, ...

k_sum, the longest chain of roundings of a row sum (the first addition to 0.f is exact and still counted):
    scalar   a lane's ceil(D / 64) additions, then the 6 levels of wave_sum                       k_sum = ceil(D / 64) + 6
    vec      (x + y) + (z + w) inside a float4: 2, `sum +=` over the NV float4: NV, the 6 levels    k_sum = 2 + NV + 6

Forward (ltrx_layernorm_fwd_kernel, ltrx_layernorm_fwd_vec_kernel + rowreg_stats, rowreg_affine)
  xsum   v = x + res * scale.  p = 0: one addition, compared bit for bit with fl32(x + res); a dropped element (scale 0): x + 0 = x
         bit for bit; else a product and an addition: gam(2) (|x| + |res scale|).  Without res v = x.
         mean, rstd and y are referred to the v the kernel WROTE (or x): that is the row it normalises.
  mean   fl(S / D): the chain and the division                                                  bar_mean = gam(k_sum + 1) mean|v|
         A constant row c whose multiples c j, j <= D, are all fp32 numbers is summed exactly in any order and D c / D = c is
         exact: bar_mean = 0 (the 1.25 row of the table; without this the row's bar would exceed eps and say nothing).
  rstd   d_c = fl(v_c - mean^) = xc_c - delta + rho_c with |delta| <= bar_mean, |rho_c| <= u (|xc_c| + bar_mean) =: rho, so
         |d_c - xc_c| <= e_c = bar_mean + rho_c.  Because sum xc = 0 the uniform shift enters the sum of squares only as D delta^2:
             |sum d^2 - sum xc^2| <= A = D bar_mean^2 + sum (2 (|xc| + bar_mean) rho + rho^2)
         the squares and the chain: gam(k_sum + 1) (Q + A), Q = sum xc^2; the division by D - 1 one more; so
             E_var = (A + gam(k_sum + 2) (Q + A)) / (D - 1)
         sqrt: |sqrt(p) - sqrt(q)| <= min(|p - q| / sqrt(q), sqrt|p - q|), and its rounding      d_std = min(..) + u (std + min(..))
         + eps: one rounding                                                                    d_den = d_std + u (den + d_std)
         precondition (asserted): d_den < den = std + eps
         1 / den^: |1 / den^ - 1 / den| <= d_den / (den (den - d_den)), and its rounding         bar_r = that + u (r + that)
  y      fl(fl(a fl(d r^)) + b): the propagated |a| (e (r + bar_r) + |xc| bar_r), three roundings on |a| (|xc| + e) (r + bar_r) + |b|

Backward (ltrx_layernorm_bwd_kernel, ltrx_layernorm_bwd_vec_kernel + LTRX_ROWREG_BWD_ACC, rowreg_bwd_coef, rowreg_bwd_dx), on the fp32
mean and rstd it is handed, as data: xc = xsum - mean, r = rstd, stdv = 1 / r - eps exactly.
  gm     g = fl(dy a): 1, the chain, the division                                               bar_gm = gam(k_sum + 2) mean|g|
  tc     r r <g, xc> / ((D - 1) stdv).  <g, xc>: g 1, fl(xsum - mean) 1, the product 1, the chain k_sum; r r, times the dot,
         (D - 1) stdv^ and the division: 4; stdv^ = fl(fl(1 / r) - eps) is off by u (stdv + eps) from the reciprocal and u stdv from
         the subtraction: relatively at most rel_s = 2 u (stdv + eps) / stdv (the cancellation against eps).  Against
         tc_abs = r^2 sum|g xc| / ((D - 1) stdv):                    bar_tc = tc_abs ((1 + gam(k_sum + 7)) / (1 - rel_s) - 1)
         precondition (asserted): every row has rel_s < 2^-6 or xc == 0 in every column (then <g, xc> = 0 exactly in the kernel
         and in the reference whichever way the stdv > 0 guard falls)
  dx     fl(fl(r fl(g^ - gm^)) - fl(tc^ xc^)) (+ dres: one more rounding on everything, n = 1, else n = 0)
         r g: g 1, the subtraction 1, the product 1, the outer subtraction 1           gam(4 + n) r |g|
         r gm: the subtraction, the product, the outer subtraction                    gam(3 + n) r (|gm| + bar_gm)
         tc xc: xc 1, the product, the outer subtraction                              gam(3 + n) (tc_abs + bar_tc) |xc|
         dres: the addition                                                           gam(1) |dres|
         (the register kernels store g = fl(dy a) before it enters gsum, the dot and dx, so its rounding is counted on every path
         through g; the scalar kernel may contract dy a - gm into one fma and then has one rounding less)
         propagated: (1 + gam(3 + n)) (r bar_gm + bar_tc |xc|)
  da, db per row the term fl(dy fl(xc^ r)): 3 roundings, dy itself none.  The chain of a partial row [da | db] of workgroup b (rows r with
         (r // wpb) % grid == b): a wave adds one row per trip of the row walk, trips = ceil(rows / (grid wpb)), then the wpb spilled
         rows are added in wave order:                                                k_part = trips + wpb
             bar_part = gam(k_part + 3) sum|dy xc r|,  gam(k_part) sum|dy|   over the rows of that workgroup
         reduced by ltrx_layernorm_bwd_reduce_kernel (a wave adds every 16th partial row, then the 16 wave sums in order):
                                                                                      k = k_part + ceil(grid / 16) + 16
         reduced by ltrx_reduce_group (reduce_cols: a wave adds every 4th row, then (0 + 1) + (2 + 3)):
                                                                                      k = k_part + ceil(grid / 4) + 2
  A fused multiply-add only removes a rounding; division and square root are the correctly rounded ones.
"""
import os
import re
from collections import namedtuple

import numpy as np

from oracle import dropout_oracle as DO
from oracle import model_oracle as MO
from tests.step_ref import F, ONE, U, _lane_sums, _wave_sum, f64, gam, over, spread, w, worst  # noqa: F401  (re-exported)

SEED, WORD = 77, 3
# restated from csrc/ltrx_layernorm.hip; tests/test_layernorm_ref_cpu.py holds them to the source (source_constants)
LN_BWD_G16 = 256
WIDE_ROWS = 16 * 4 * LN_BWD_G16
FWD_GRID_CAP, BWD_GRID_CAP = 1024, 320
MAX_BWD_D = 2048                                        # 4 waves x 2 x D floats of dynamic LDS = 64 KiB


def source_constants():
    """the same numbers read from the source text"""
    here = os.path.dirname(os.path.abspath(__file__))
    src = open(os.path.join(here, "..", "allrank_amd", "csrc", "ltrx_layernorm.hip")).read()
    hdr = open(os.path.join(here, "..", "allrank_amd", "csrc", "ltrx_rowreg.h")).read()
    g16 = int(re.search(r"#define LTRX_LN_BWD_G16 (\d+)", src).group(1))
    assert re.search(r"#define LTRX_LN_BWD_WIDE_ROWS \(16 \* 4 \* LTRX_LN_BWD_G16\)", src)
    grid = lambda name, per: int(re.search(  # noqa: E731
        r"static int %s\(int rows\) \{\s*int g = \(rows \+ %d\) / %d;\s*return g > (\d+) \? \1 :" % (name, per - 1, per), src).group(1))
    wide = re.search(r"ln_bwd_wide\(int rows, int D\) \{ return D <= (\d+) && rows >= LTRX_LN_BWD_WIDE_ROWS; \}", src)
    vec = re.search(r"return D % (\d+) == 0 && D <= (\d+) && \(\(\(uintptr_t\)p0 \| \(uintptr_t\)p1 \| \(uintptr_t\)p2\) & (\d+)\) == 0;", hdr)
    assert re.search(r"LnBwdShape\{LTRX_LN_BWD_G16, 16\} : LnBwdShape\{ln_bwd_grid\(rows\), 4\}", src)
    assert re.search(r"\(size_t\)4 \* 2 \* D \* sizeof\(float\) > 64 \* 1024\) return LTRX_EUNSUPPORTED", src)
    return dict(g16=g16, wide_rows=16 * 4 * g16, fwd_cap=grid("ln_grid", 4), fwd_vec_cap=grid("ln_fwd_vec_grid", 8),
                bwd_cap=grid("ln_bwd_grid", 16), wide_max_d=int(wide.group(1)), vec_mod=int(vec.group(1)), vec_max_d=int(vec.group(2)),
                vec_align=int(vec.group(3)) + 1, max_bwd_d=64 * 1024 // (4 * 2 * 4))


def ln_vec_ok(D, addresses=()):
    """the register arm's predicate: the width and every (non-NULL) pointer's address"""
    return D % 256 == 0 and D <= 1024 and all(int(p) % 16 == 0 for p in addresses)


def fwd_grid(rows, vec):
    per = 8 if vec else 4
    return max(1, min(FWD_GRID_CAP, -(-rows // per)))


def ln_bwd_shape(rows, D, vec):
    """(grid, waves per workgroup) of the backward launch == the number of partial rows, and how rows map to them"""
    if vec and D <= 512 and rows >= WIDE_ROWS:
        return LN_BWD_G16, 16
    return max(1, min(BWD_GRID_CAP, -(-rows // 16))), 4


def workspace_bytes(rows, D):
    return max(LN_BWD_G16, BWD_GRID_CAP) * 2 * D * 4 if rows > 0 and D > 0 else 0


def fwd_kernel(D, vec):
    return "ltrx_layernorm_fwd_vec_kernel<%d>" % (D // 256) if vec else "ltrx_layernorm_fwd_kernel"


def bwd_kernel(rows, D, vec):
    return "ltrx_layernorm_bwd_vec_kernel<%d, %d>" % (D // 256, ln_bwd_shape(rows, D, vec)[1]) if vec else "ltrx_layernorm_bwd_kernel"


ALL_KERNELS = (["ltrx_layernorm_fwd_kernel", "ltrx_layernorm_bwd_kernel"] + ["ltrx_layernorm_fwd_vec_kernel<%d>" % n for n in (1, 2, 3, 4)]
               + ["ltrx_layernorm_bwd_vec_kernel<%d, 4>" % n for n in (1, 2, 3, 4)] + ["ltrx_layernorm_bwd_vec_kernel<%d, 16>" % n for n in (1, 2)])


def k_sum(D, vec):
    return 2 + D // 256 + 6 if vec else -(-D // 64) + 6


# ---------------------------------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------------------------------
def keep_scale(p, seed, word, rows, D):
    """the residual's dropout multipliers (0 or 1 / (1 - p), fp32), None for p = 0; word None: no drop_step pointer"""
    return DO.keep_scale(p, seed, 0 if word is None else word, (rows, D)) if p > 0 else None


def xsum_ref(x, res, scale):
    if res is None:
        return f64(x)
    if scale is None:
        return f64(np.asarray(x, F) + np.asarray(res, F))                      # one fp32 addition: compared bit for bit
    return f64(x) + f64(res) * f64(scale)


def xsum_bar(x, res, scale):
    if res is None or scale is None:
        return np.zeros(np.asarray(x).shape)
    return np.where(np.asarray(scale) == 0, 0.0, gam(2) * (np.abs(f64(x)) + np.abs(f64(res) * f64(scale))))


def fwd_ref(v, a, b, eps):
    """(mean, rstd, y) of the rows v in fp64: oracle/model_oracle.py's custom_ln_fwd"""
    y, (xc, std, r, xhat) = MO.custom_ln_fwd(f64(v), f64(a), f64(b), w(eps))
    return f64(v).mean(-1), r[:, 0], y


def _exact_rows(v):
    """rows that are constant = c with every c j, j <= D, an fp32 number: any summation order is exact"""
    D = v.shape[1]
    const = (v == v[:, :1]).all(1)
    mult = v[const, :1] * np.arange(1, D + 1)[None, :]
    out = np.zeros(v.shape[0], bool)
    out[np.flatnonzero(const)] = (mult.astype(F).astype(np.float64) == mult).all(1)
    return out


def fwd_bar(v, a, b, eps, vec):
    """(bar_mean, bar_rstd, bar_y)"""
    v, a, b, eps = f64(v), f64(a), f64(b), w(eps)
    D = v.shape[1]
    k = k_sum(D, vec)
    mean = v.mean(-1, keepdims=True)
    bar_mean = gam(k + 1) * np.abs(v).mean(-1, keepdims=True)
    bar_mean[_exact_rows(v)] = 0.0
    xc = np.abs(v - mean)
    rho = U * (xc + bar_mean)
    e = bar_mean + rho
    Q = (xc * xc).sum(-1, keepdims=True)
    A = D * bar_mean ** 2 + (2 * (xc + bar_mean) * rho + rho * rho).sum(-1, keepdims=True)
    E_var = (A + gam(k + 2) * (Q + A)) / (D - 1)
    std = np.sqrt(Q / (D - 1))
    with np.errstate(divide="ignore", invalid="ignore"):
        d_std = np.minimum(np.where(std > 0, E_var / std, np.inf), np.sqrt(E_var))
    d_std = d_std + U * (std + d_std)
    den = std + eps
    d_den = d_std + U * (den + d_std)
    assert (d_den < den).all(), "the bound on std + eps reaches std + eps: the bar of rstd says nothing"
    r = 1.0 / den
    bar_r = d_den / (den * (den - d_den))
    bar_r = bar_r + U * (r + bar_r)
    bar_y = np.abs(a) * (e * (r + bar_r) + xc * bar_r) + gam(3) * (np.abs(a) * (xc + e) * (r + bar_r) + np.abs(b))
    return bar_mean[:, 0], bar_r[:, 0], bar_y


FWD_WRONG = ("biased", "eps_inside", "mean_padded", "sq_tail_dropped", "res_after_stats", "scale_on_x")


def _row_sum(t, vec):
    """[rows, D] -> [rows] in the kernels' order"""
    if not vec:
        return _lane_sums(t)
    rows, D = t.shape
    q = t.reshape(rows, D // 256, 64, 4)
    acc = np.zeros((rows, 64), F)
    for i in range(D // 256):
        acc = acc + ((q[:, i, :, 0] + q[:, i, :, 1]) + (q[:, i, :, 2] + q[:, i, :, 3]))
    return _wave_sum(acc)


def fwd_f32(x, res, scale, a, b, eps, vec, wrong=None):
    """(xsum, mean, rstd, y) as the kernels compute them"""
    x, a, b, eps = np.asarray(x, F), np.asarray(a, F), np.asarray(b, F), F(eps)
    D = x.shape[1]
    if res is None:
        v = x
    elif scale is None:
        v = x + np.asarray(res, F)
    else:
        v = (x + np.asarray(res, F)) * scale if wrong == "scale_on_x" else x + np.asarray(res, F) * scale
    s = x if wrong == "res_after_stats" else v
    mean = _row_sum(s, vec) / F(64 * -(-D // 64) if wrong == "mean_padded" else D)
    d = s - mean[:, None]
    dd = d * d
    if wrong == "sq_tail_dropped":
        dd[:, D - D % 64:] = 0
    var = _row_sum(dd, vec) / F(D if wrong == "biased" else D - 1)
    r = ONE / np.sqrt(var + eps) if wrong == "eps_inside" else ONE / (np.sqrt(var) + eps)
    y = a * ((v - mean[:, None]) * r[:, None]) + b
    return v, mean, r, y


# ---------------------------------------------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------------------------------------------
def _by_partial(t, grid, wpb):
    """[rows, D] fp64 -> [grid, D]: partial row b sums the rows r with (r // wpb) % grid == b"""
    rows, D = t.shape
    trips = -(-rows // (grid * wpb))
    pad = np.zeros((trips * grid * wpb, D))
    pad[:rows] = t
    return pad.reshape(trips, grid, wpb, D).sum((0, 2))


def bwd_ref(dy, xsum, a, mean, rstd, dres, eps, shape=None):
    """dx, da, db (and the partial rows [grid, 2, D] of launch shape (grid, wpb)) in fp64 from the statistics handed in:
    custom_ln_bwd on the cache those statistics stand for"""
    dy, a, r = f64(dy), f64(a), f64(rstd)[:, None]
    xc = f64(xsum) - f64(mean)[:, None]
    std = 1.0 / r - w(eps)
    grads = {}
    dx = MO.custom_ln_bwd((xc, std, r, xc * r), a, dy, grads, "n")
    if dres is not None:
        dx = dx + f64(dres)
    out = dict(dx=dx, da=grads["n.a_2"], db=grads["n.b_2"])
    if shape is not None:
        out["partial"] = np.stack([_by_partial(dy * (xc * r), *shape), _by_partial(dy, *shape)], 1)
    return out


def k_partial(rows, grid, wpb):
    return -(-rows // (grid * wpb)) + wpb


def k_reduce(grid, reducer):
    return -(-grid // 16) + 16 if reducer == "kernel" else -(-grid // 4) + 2


def bwd_bar(dy, xsum, a, mean, rstd, dres, eps, vec, shape):
    """dict(dx, partial, da / db reduced by ltrx_layernorm_bwd_reduce_kernel, da_group / db_group by ltrx_reduce_group)"""
    dy, a, r, eps = f64(dy), f64(a), f64(rstd)[:, None], w(eps)
    rows, D = dy.shape
    k = k_sum(D, vec)
    xc = f64(xsum) - f64(mean)[:, None]
    g = dy * a
    gm = np.abs(g.mean(-1, keepdims=True))
    bar_gm = gam(k + 2) * np.abs(g).mean(-1, keepdims=True)
    flat = (xc == 0).all(1, keepdims=True)
    stdv = 1.0 / r - eps
    with np.errstate(divide="ignore", invalid="ignore"):
        rel_s = np.where(flat, 0.0, 2 * U * (stdv + eps) / stdv)
        tc_abs = np.where(flat, 0.0, r * r * np.abs(g * xc).sum(-1, keepdims=True) / ((D - 1) * stdv))
    assert (flat | ((stdv > 0) & (rel_s < 2.0 ** -6))).all(), "a row is neither clear of stdv = 0 nor exactly constant"
    bar_tc = tc_abs * ((1 + gam(k + 7)) / (1 - rel_s) - 1)
    n = 0 if dres is None else 1
    axc = np.abs(xc)
    bar_dx = (gam(4 + n) * r * np.abs(g) + gam(3 + n) * (r * (gm + bar_gm) + (tc_abs + bar_tc) * axc)
              + (1 + gam(3 + n)) * (r * bar_gm + bar_tc * axc))
    if dres is not None:
        bar_dx = bar_dx + gam(1) * np.abs(f64(dres))
    grid, wpb = shape
    kp = k_partial(rows, grid, wpb)
    sa, sb = _by_partial(np.abs(dy * (xc * r)), grid, wpb), _by_partial(np.abs(dy), grid, wpb)
    out = dict(dx=bar_dx, partial=np.stack([gam(kp + 3) * sa, gam(kp) * sb], 1))
    for reducer, tag in (("kernel", ""), ("group", "_group")):
        kr = kp + k_reduce(grid, reducer)
        out["da" + tag], out["db" + tag] = gam(kr + 3) * sa.sum(0), gam(kr) * sb.sum(0)
    return out


BWD_WRONG = ("no_gm", "D_for_Dm1", "tc_sign", "no_dres", "da_on_g", "tail_row_missing", "second_trip_shifted")


def bwd_f32(dy, xsum, a, mean, rstd, dres, eps, vec, shape, wrong=None):
    """(dx, partial rows [grid, 2, D]) as the kernels compute them"""
    dy, xs, a, eps = np.asarray(dy, F), np.asarray(xsum, F), np.asarray(a, F), F(eps)
    r = np.asarray(rstd, F)[:, None]
    rows, D = dy.shape
    xc = xs - np.asarray(mean, F)[:, None]
    g = dy * a
    gm = np.zeros((rows, 1), F) if wrong == "no_gm" else (_row_sum(g, vec) / F(D))[:, None]
    dot = _row_sum(g * xc, vec)[:, None]
    stdv = ONE / r - eps
    with np.errstate(divide="ignore", invalid="ignore"):
        tc = np.where(stdv > 0, r * r * dot / (F(D if wrong == "D_for_Dm1" else D - 1) * stdv), F(0)).astype(F)
    dx = r * (g - gm) + tc * xc if wrong == "tc_sign" else r * (g - gm) - tc * xc
    if dres is not None and wrong != "no_dres":
        dx = dx + np.asarray(dres, F)
    ta, tb = (g if wrong == "da_on_g" else dy) * (xc * r), dy
    if wrong == "tail_row_missing":
        ta, tb = ta.copy(), tb.copy()
        ta[-1], tb[-1] = 0, 0
    grid, wpb = shape
    trips = -(-rows // (grid * wpb))
    part = []
    for t in (ta, tb):
        pad = np.zeros((trips * grid * wpb, D), F)          # a wave without a row adds nothing
        pad[:rows] = t
        pad = pad.reshape(trips, grid, wpb, D)
        acc = np.zeros((grid, wpb, D), F)
        for k in range(trips):
            acc = acc + (np.roll(pad[k], 1, axis=0) if (wrong == "second_trip_shifted" and k >= 1) else pad[k])
        prow = np.zeros((grid, D), F)
        for wv in range(wpb):                               # LDS combine, wave order
            prow = prow + acc[:, wv]
        part.append(prow)
    return dx.astype(F), np.stack(part, 1)


def reduce_f32(partial, reducer):
    """[grid, 2, D] -> (da, db): ltrx_layernorm_bwd_reduce_kernel ("kernel") or ltrx_reduce_group's reduce_cols ("group")"""
    nw = 16 if reducer == "kernel" else 4
    grid = partial.shape[0]
    sh = []
    for wv in range(nw):
        acc = np.zeros(partial.shape[1:], F)
        for k in range(wv, grid, nw):
            acc = acc + partial[k]
        sh.append(acc)
    if reducer == "kernel":
        t = np.zeros(partial.shape[1:], F)
        for acc in sh:
            t = t + acc
    else:
        t = (sh[0] + sh[1]) + (sh[2] + sh[3])
    return t[0], t[1]


# ---------------------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------------------
# misaligned: None, "in" (x / dy 4 bytes off 16-byte alignment) or "out" (y / dx).  full: every forward and backward option; the large
# and the launch-shape rows take FWD_FEW / BWD_FEW: the options are properties of a row's arithmetic, not of the row walk, and the two
# of each kind kept there touch every operand (xsum given without res; res, dropout and the step word; dres with the reduce kernel;
# the partial rows and ltrx_reduce_group without dres).
Case = namedtuple("Case", "name rows D eps misaligned full")
FwdOpt = namedtuple("FwdOpt", "name res xsum p word")
BwdOpt = namedtuple("BwdOpt", "name entry dres")           # entry "partial" also sums the partial rows with ltrx_reduce_group

FWD_OPTIONS = (FwdOpt("x only", False, False, 0.0, None), FwdOpt("x only, xsum written", False, True, 0.0, None),
               FwdOpt("res, p 0", True, True, 0.0, None), FwdOpt("res, p 0.3, step word", True, True, 0.3, WORD),
               FwdOpt("res, p 0.3, no step word", True, True, 0.3, None))
FWD_FEW = (FWD_OPTIONS[1], FWD_OPTIONS[3])
BWD_OPTIONS = (BwdOpt("bwd, dres", "bwd", True), BwdOpt("bwd", "bwd", False), BwdOpt("partial, dres", "partial", True),
               BwdOpt("partial", "partial", False))
BWD_FEW = (BWD_OPTIONS[0], BWD_OPTIONS[3])


def _cases():
    out = []

    def add(rows, D, eps, misaligned=None, full=True):
        name = "%dx%d eps %g%s" % (rows, D, eps, "" if misaligned is None else " misaligned " + misaligned)
        out.append(Case(name, rows, D, eps, misaligned, full))

    for eps in (1e-6, 1e-3):
        for D in (2, 3, 65, 136, 1280, 2048, 256, 512, 768, 1024):                       # scalar widths, then the register layout's
            for rows in (1, 3, 37):
                add(rows, D, eps)
        add(37, 512, eps, "in")
        add(37, 512, eps, "out")
    for eps in (1e-6, 1e-3):
        for D in (136, 768, 1024):             # above the forward grid cap (1024 x 4 rows; vec 1024 x 8: the wide rows) and the backward's 320 x 16
            add(5127, D, eps, full=False)
        for D in (256, 512):
            add(WIDE_ROWS - 1, D, eps, full=False)                                       # four waves, just below the switch
            add(WIDE_ROWS + 5, D, eps, full=False)                                       # sixteen waves (the flagship step's shape); the vec forward's third trip
    add(WIDE_ROWS + 5, 1024, 1e-6, full=False)                                           # four waves, 13 trips (tests/test_gpu_norm_head.py)
    for rows in (32, 160, 1056):                                                         # the launch shapes of tests/test_gpu_tn_group_ln.py
        for D in (256, 512, 768):
            add(rows, D, 1e-6, full=False)
    add(1056, 1024, 1e-6, full=False)
    return out


CASES = _cases()
LARGE = 1 << 21                                       # rows x D from which a case gets parametrised ids of its own per call


def is_vec(c):
    return ln_vec_ok(c.D) and c.misaligned is None


def fwd_options(c):
    return FWD_OPTIONS if c.full else FWD_FEW


def bwd_options(c):
    return BWD_OPTIONS if c.full else BWD_FEW


def kernels(c):
    v = is_vec(c)
    return {fwd_kernel(c.D, v), bwd_kernel(c.rows, c.D, v)}


CONST_ROW, BIG_ROW, TINY_ROW, NEAR_ROW, ZERO_DY_ROW = 1, 2, 3, 4, 5


def inputs(c):
    """dict(x, res, a, b, dy, dres): 2 N(0, 1) + 0.3 with, where there are rows for them (never the last row), one constant row 1.25
    (its fp32 sum is exact), one row 1e4 + N(0, 1), one row 1e-6 N(0, 1) (std at the size of eps), one row 3 + 1e-4 N(0, 1), one zero
    in a, one all-zero dy row, dy over the binades 2^-4 .. 2^4.  The residual of a special row is at that row's scale.  The misaligned
    cases share the data of the aligned 37 x 512 case."""
    rows, D = c.rows, c.D
    rng = np.random.default_rng([rows, D, int(round(-np.log10(c.eps)))])
    n = lambda: rng.standard_normal((rows, D))        # noqa: E731
    x, res = 2 * n() + 0.3, 2 * n() + 0.3
    if rows - 1 > CONST_ROW:
        x[CONST_ROW], res[CONST_ROW] = 1.25, 0.0
    if rows - 1 > BIG_ROW:
        x[BIG_ROW] = 1e4 + rng.standard_normal(D)
    if rows - 1 > TINY_ROW:
        x[TINY_ROW], res[TINY_ROW] = 1e-6 * rng.standard_normal(D), 1e-6 * rng.standard_normal(D)
    if rows - 1 > NEAR_ROW:
        x[NEAR_ROW], res[NEAR_ROW] = 3 + 1e-4 * rng.standard_normal(D), 1e-4 * rng.standard_normal(D)
    a, b = 1 + 0.1 * rng.standard_normal(D), 0.1 * rng.standard_normal(D)
    a[min(3, D - 1)] = 0.0
    dy = spread(rng, rows * D, -4, 4).reshape(rows, D)
    if rows - 1 > ZERO_DY_ROW:
        dy[ZERO_DY_ROW] = 0.0
    return dict(x=x.astype(F), res=res.astype(F), a=a.astype(F), b=b.astype(F), dy=dy, dres=rng.standard_normal((rows, D)).astype(F))


def fwd_applies(c, opt, wrong):
    """None if the defect shows on this case under this forward option, else why it cannot"""
    if wrong in ("mean_padded", "sq_tail_dropped") and c.D % 64 == 0:
        return "D is a multiple of 64: no partial last trip of the lanes"
    if wrong in ("res_after_stats", "scale_on_x") and not opt.res:
        return "no residual"
    if wrong == "scale_on_x" and opt.p == 0:
        return "no dropout scale"
    if wrong == "eps_inside" and c.eps < 1e-4 and c.rows - 1 <= CONST_ROW:
        return "eps 1e-6 against ordinary rows only: sqrt(var + eps) is within the bar of std + eps (0.4 of it)"
    return None


def tc_shift(dy, xsum, a, mean, rstd, eps):
    """what D for D - 1 in tc moves dx by, exactly: |tc xc| / D.  <g, xc> is a sum that cancels: where chance makes it small in every
    row of a case (one wide row), the defect is below the roundings of the other terms and no bar can tell"""
    r = f64(rstd)[:, None]
    xc = f64(xsum) - f64(mean)[:, None]
    D = xc.shape[1]
    stdv = 1.0 / r - w(eps)
    with np.errstate(divide="ignore", invalid="ignore"):
        tc = np.where((xc == 0).all(1, keepdims=True), 0.0, r * r * (f64(dy) * f64(a) * xc).sum(-1, keepdims=True) / ((D - 1) * stdv))
    return np.abs(tc * xc) / D


def bwd_applies(c, opt, wrong, shift=None, bar_dx=None):
    """None if the defect shows on this case under this backward option, else why it cannot (shift, bar_dx: tc_shift and the bar of
    dx, for the one defect whose size depends on the data)"""
    grid, wpb = ln_bwd_shape(c.rows, c.D, is_vec(c))
    if wrong == "D_for_Dm1" and shift is not None and not (shift > 2 * bar_dx).any():
        return "<g, xc> cancels: tc / D is within twice the bar of dx on every entry"
    if wrong == "no_dres" and not opt.dres:
        return "no residual gradient"
    if wrong == "second_trip_shifted" and (c.rows <= grid * wpb or grid == 1):
        return "one trip of the row walk (or one workgroup)"
    return None
