"""fp64 references, a-priori bars and fp32 transcriptions of the optimizer and glue kernels of the explicit training step
(allrank_amd/csrc/ltrx_train.hip, ltrx_extras.hip)  --  TEST INFRASTRUCTURE, plain numpy, needs no GPU.

For every operation there are three functions that take the fp32 inputs exactly as the kernel receives them:

    *_ref   the operation in fp64.  Hyperparameters are the fp32 values the C ABI receives, widened (``w``): that is the rule
            the kernel implements.  (``hyper=float`` keeps them Python doubles: the form that is compared with torch.)
    *_bar   the bound on |kernel - *_ref| for ONE call from identical fp32 state.  With u = 2^-24 (``U``) a bar is
            (fp32 roundings on the longest path) * u * (sum of the absolute values of the terms that are added); ``gam(k)`` =
            k u / (1 - k u) is that count with the higher-order terms kept.  A reduction of T terms in any order costs T - 1.
            No bar holds a measured number.
    *_f32   the kernel's arithmetic in np.float32, in the operation order of the source (and the grid-stride / wave order of the
            sums): tests/test_step_ref_cpu.py shows that it meets the bar, and that each ``wrong=`` variant of it does not.

powf, expf and tanhf are documented by HIP at 1 ulp; 1 ulp is at most 2 u relative, hence the allowance ``P_LIBM`` = 2 (in units
of u).  The bars assume that no intermediate falls below the smallest normal fp32 number; where a result itself can (the
saturated output activations) the bar carries FLT_MIN, below which fp32 has no relative precision.  The division and square root
of the device code are the correctly rounded ones (one rounding each); a fused multiply-add only removes a rounding.
"""
import numpy as np

from oracle import model_oracle as MO

U = 2.0 ** -24
P_LIBM = 2.0
FLT_MIN = 2.0 ** -126
FLT_MAX = np.float32(3.4028234663852886e38)
DENORM = np.float32(1e-41)
NO_SEGMENT = 0x7fffffff
F = np.float32
ONE = np.float32(1.0)


def gam(k):
    return k * U / (1.0 - k * U)


def w(x):
    """a hyperparameter as the C ABI receives it: rounded to fp32, widened to a Python double"""
    return float(np.float32(x))


def f64(a):
    return np.asarray(a, np.float64)


def over(got, ref, bar):
    """True where an entry is outside its bar (a non-finite entry always is)"""
    with np.errstate(invalid="ignore"):
        return ~(np.abs(f64(got) - f64(ref)) <= f64(bar))


def worst(got, ref, bar):
    """largest error / bar (0 / 0 counts as 0, anything over a zero bar as inf)"""
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(f64(got) - f64(ref))
        r = np.where(f64(bar) > 0, err / f64(bar), np.where(err == 0, 0.0, np.inf))
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max()) if r.size else 0.0


def spread(rng, n, lo, hi):
    """N(0, 1) times 2^k, k uniform in [lo, hi] per element: operands that span many binades"""
    return (rng.standard_normal(n) * 2.0 ** rng.integers(lo, hi + 1, n)).astype(F)


def _wave_sum(x):
    """[..., 64] -> [...]: the pairwise tree of a wave's DPP reduction"""
    for _ in range(6):
        x = x[..., 0::2] + x[..., 1::2]
    return x[..., 0]


# ---------------------------------------------------------------------------------------------------------------------------------
# Adam / AdamW (ltrx_adam_kernel).  t is the step count AFTER the bump, i.e. the one the bias corrections use.
#
#   s   = gs * gsd                                   1 rounding
#   gr  = g s + l2 p                                 term g s: s, product, add = 3; term l2 p: product, add = 2
#         -> |gr^ - gr| <= gam(3) G,  G = |g s| + |l2 p|
#   m'  = b1 m + (1 - b1) gr                         b1 m: 2;  (1 - b1) gr: subtraction, product, add + the 3 of gr = 6
#         -> bar_m = gam(6) (|b1 m| + (1 - b1) G)
#   v'  = b2 v + (1 - b2) gr gr                      b2 v: 2;  the other: subtraction, 2 products, add + 2 * 3 of gr = 10
#         -> bar_v = gam(10) (b2 v + (1 - b2) G^2)
#   p'  = p shrink - ss m' / den,   ss = lr / bc1,  den = sqrt(v') / bc2s + eps,  bc1 = 1 - b1^t,  bc2s = sqrt(1 - b2^t)
#     p shrink: lr wd, 1 - ., product, final subtraction = 4                              -> gam(4) |p shrink|
#     update Upd = ss m' / den:
#       m' carries bar_m, v' carries bar_v:  |sqrt(v'^) - sqrt(v')| <= min(bar_v / sqrt(v'), sqrt(bar_v)) =: d_rt (exact: the
#       difference of two square roots), d_den = d_rt / bc2s, and with den_lo = max(den - d_den, eps)
#           E = ss bar_m / den_lo + |Upd| d_den / den_lo
#       its own roundings, all relative to |Upd| because den adds non-negative terms: the subtractions 1 - b1^t and 1 - b2^t (the
#       latter halved by the sqrt, counted whole), sqrt for bc2s, lr / bc1, sqrt(v'), / bc2s, + eps, m' / den, ss * ., the final
#       subtraction = 10                                                                 -> gam(10) |Upd|
#       the conditioning of the bias corrections: powf is off by P u b^t, 1 - b^t by that, relatively P u b^t / (1 - b^t); the
#       sqrt halves it for b2                                     -> P u (b1^t / (1 - b1^t) + 0.5 b2^t / (1 - b2^t)) |Upd|
#   bar_p = gam(4) |p shrink| + (gam(10) + cond) |Upd| + (1 + gam(10) + cond) E
# The amplification b^t / (1 - b^t) is a property of computing the corrections in fp32: 4 at t = 1 for b1 = 0.8 but 999 for b2 =
# 0.999 at t = 1 and 499 at t = 2; it is below 1 from t = 693 on.
# ---------------------------------------------------------------------------------------------------------------------------------
def _adam_hyper(lr, b1, b2, eps, wd, gs, gsd, hyper):
    s = hyper(gs) * (1.0 if gsd is None else hyper(gsd))
    return hyper(lr), hyper(b1), hyper(b2), hyper(eps), hyper(wd), s


def adam_ref(p, g, m, v, t, lr, b1, b2, eps, wd, decoupled, gs=1.0, gsd=None, hyper=w):
    """(p', m', v') in fp64 through oracle/model_oracle.py's Adam"""
    lr, b1, b2, eps, wd, s = _adam_hyper(lr, b1, b2, eps, wd, gs, gsd, hyper)
    opt = MO.Adam({"x": f64(p)}, lr, b1, b2, eps, wd, bool(decoupled))
    opt.t = int(t) - 1
    opt.m["x"], opt.v["x"] = f64(m).copy(), f64(v).copy()
    params = {"x": f64(p).copy()}
    opt.step(params, {"x": f64(g) * s})
    return params["x"], opt.m["x"], opt.v["x"]


def adam_bar(p, g, m, v, t, lr, b1, b2, eps, wd, decoupled, gs=1.0, gsd=None):
    p, g, m, v = f64(p), f64(g), f64(m), f64(v)
    pn, mn, vn = adam_ref(p, g, m, v, t, lr, b1, b2, eps, wd, decoupled, gs, gsd)
    lr, b1, b2, eps, wd, s = _adam_hyper(lr, b1, b2, eps, wd, gs, gsd, w)
    l2, shrink = (0.0, 1.0 - lr * wd) if decoupled else (wd, 1.0)
    G = np.abs(g * s) + np.abs(l2 * p)
    bar_m = gam(6) * (np.abs(b1 * m) + (1 - b1) * G)
    bar_v = gam(10) * (b2 * v + (1 - b2) * G * G)
    bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
    ss, bc2s = lr / bc1, np.sqrt(bc2)
    rt = np.sqrt(vn)
    with np.errstate(divide="ignore", invalid="ignore"):
        d_rt = np.minimum(np.where(rt > 0, bar_v / rt, np.inf), np.sqrt(bar_v))
    den = rt / bc2s + eps
    d_den = d_rt / bc2s
    den_lo = np.maximum(den - d_den, eps)
    upd = np.abs(ss * mn / den)
    E = ss * bar_m / den_lo + upd * d_den / den_lo
    cond = P_LIBM * U * (b1 ** t / bc1 + 0.5 * b2 ** t / bc2)
    bar_p = gam(4) * np.abs(p * shrink) + (gam(10) + cond) * upd + (1 + gam(10) + cond) * E
    return bar_p, bar_m, bar_v


ADAM_WRONG = ("swap_decay", "eps_inside", "no_bc1", "t_minus_1", "no_dev_scale", "scale_after_decay")


def adam_f32(p, g, m, v, t, lr, b1, b2, eps, wd, decoupled, gs=1.0, gsd=None, wrong=None):
    p, g, m, v = (np.asarray(a, F) for a in (p, g, m, v))
    lr, b1, b2, eps, wd, scale = F(lr), F(b1), F(b2), F(eps), F(wd), F(gs)
    if wrong == "swap_decay":                      # AdamW run as L2 and L2 run as AdamW
        decoupled = not decoupled
    l2, shrink = (F(0), ONE - lr * wd) if decoupled else (wd, ONE)
    if gsd is not None and wrong != "no_dev_scale":
        scale = scale * F(gsd)
    tt = F(t - 1 if wrong == "t_minus_1" else t)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        bc1 = ONE if wrong == "no_bc1" else ONE - np.power(b1, tt)
        bc2s = np.sqrt(ONE - np.power(b2, tt))
        ss = lr / bc1
        gr = (g + l2 * p) * scale if wrong == "scale_after_decay" else g * scale + l2 * p
        mn = b1 * m + (ONE - b1) * gr
        vn = b2 * v + (ONE - b2) * gr * gr
        den = (np.sqrt(vn) + eps) / bc2s if wrong == "eps_inside" else np.sqrt(vn) / bc2s + eps
        pn = p * shrink - ss * (mn / den)
    return pn, mn, vn


ADAM_SIZES = (1, 3, 4, 7, 1027)
ADAM_BIG = 2097152 + 3 * 1024 + 3                  # above the grid cap (2048 blocks x 256 threads x 4), with a scalar tail of 3
ADAM_STEPS = (0, 1, 2, 9, 999, 99999)              # the device step count BEFORE the call
ADAM_BETAS = ((0.8, 0.95, 1e-6), (0.9, 0.999, 1e-8))


def adam_configs():
    out = []
    for (b1, b2, eps) in ADAM_BETAS:
        for decoupled in (0, 1):
            for gsd in (None, 0.37):
                for t0 in ADAM_STEPS:
                    out.append(dict(lr=3e-3, b1=b1, b2=b2, eps=eps, wd=0.1, decoupled=decoupled, gs=0.5, gsd=gsd, t0=t0))
    return out


def adam_big_configs():
    c = adam_configs()
    pick = lambda b1, dec, dev, t0: [k for k in c if k["b1"] == b1 and k["decoupled"] == dec and (k["gsd"] is not None) == dev and k["t0"] == t0][0]
    return [pick(0.8, 0, True, 2), pick(0.8, 1, False, 999), pick(0.9, 0, False, 99999)]


def adam_inputs(rng, n):
    """p, g, m, v: gradients and moments over the binades 2^-26 .. 2^4 (down to eps), parameters over 2^-6 .. 2^6"""
    return spread(rng, n, -6, 6), spread(rng, n, -26, 4), spread(rng, n, -26, 4), spread(rng, n, -26, 4) ** 2


def adam_args(cfg):
    """the keyword arguments of adam_ref / adam_bar / adam_f32 for one configuration"""
    k = dict(cfg)
    k["t"] = k.pop("t0") + 1
    return k


# ---------------------------------------------------------------------------------------------------------------------------------
# SGD (ltrx_sgd_kernel; dampening 0)
#   gr = g s + wd p                 as for Adam: gam(3) G, G = |g s| + |wd p|
#   b  = mom buf + gr               mom buf: 2; gr: 3 + 1 = 4           -> bar_buf = gam(4) (|mom buf| + G)
#   d  = gr (3) | b (4) | gr + mom b (nesterov: b's 4, product, add = 6), with A = G | |mom buf| + G | G + |mom| (|mom buf| + G)
#   p' = p - lr d                   product and subtraction more         -> bar_p = gam(k_d + 2) (|p| + lr A)
# ---------------------------------------------------------------------------------------------------------------------------------
def sgd_ref(p, g, buf, lr, mom, nesterov, wd, gs=1.0, gsd=None, hyper=w):
    p, g = f64(p), f64(g)
    lr, mom, wd = hyper(lr), hyper(mom), hyper(wd)
    s = hyper(gs) * (1.0 if gsd is None else hyper(gsd))
    gr = g * s + wd * p
    bn = None
    if mom != 0:
        bn = mom * f64(buf) + gr
        gr = gr + mom * bn if nesterov else bn
    return p - lr * gr, bn


def sgd_bar(p, g, buf, lr, mom, nesterov, wd, gs=1.0, gsd=None):
    p, g = f64(p), f64(g)
    lr, mom, wd = w(lr), w(mom), w(wd)
    s = w(gs) * (1.0 if gsd is None else w(gsd))
    G = np.abs(g * s) + np.abs(wd * p)
    if mom == 0:
        return gam(5) * (np.abs(p) + lr * G), None
    B = np.abs(mom * f64(buf)) + G
    if nesterov:
        return gam(8) * (np.abs(p) + lr * (G + abs(mom) * B)), gam(4) * B
    return gam(6) * (np.abs(p) + lr * B), gam(4) * B


SGD_WRONG = ("plain_momentum", "decay_after_momentum", "dampening", "no_dev_scale")


def sgd_f32(p, g, buf, lr, mom, nesterov, wd, gs=1.0, gsd=None, wrong=None):
    p, g = np.asarray(p, F), np.asarray(g, F)
    lr, mom, wd, scale = F(lr), F(mom), F(wd), F(gs)
    if gsd is not None and wrong != "no_dev_scale":
        scale = scale * F(gsd)
    late = wrong == "decay_after_momentum"
    gr = g * scale if late else g * scale + wd * p
    bn = None
    if mom != 0:
        bn = mom * np.asarray(buf, F) + ((ONE - mom) * gr if wrong == "dampening" else gr)
        gr = gr + mom * bn if (nesterov and wrong != "plain_momentum") else bn
    if late:
        gr = gr + wd * p
    return p - lr * gr, bn


SGD_SIZES = (1, 5, 1048576 + 259)                  # the last: above the grid cap (4096 blocks x 256 threads)
SGD_MODES = (dict(mom=0.0, nesterov=0, wd=0.0), dict(mom=0.9, nesterov=0, wd=0.0), dict(mom=0.9, nesterov=1, wd=0.05),
             dict(mom=0.0, nesterov=0, wd=0.05))


def sgd_configs():
    return [dict(lr=0.02, gs=0.5, gsd=gsd, **mode) for mode in SGD_MODES for gsd in (None, 0.37)]


def sgd_inputs(rng, n):
    return spread(rng, n, -6, 6), spread(rng, n, -20, 6), spread(rng, n, -20, 6)


# ---------------------------------------------------------------------------------------------------------------------------------
# clip_grad_norm_ (ltrx_sumsq_partial_kernel + ltrx_clip_scale_kernel)
#   S = sum g^2 in any order: the products and n - 1 additions    -> relative gam(n)   (every term is non-negative)
#   norm = sqrt(S): |sqrt(1 + x) - 1| <= |x| / (2 - |x|), and the sqrt's own rounding  -> rel_n = gam(n) / (2 - gam(n)) + u (1 + ..)
#   c = max_norm / (norm + 1e-6f): the addition and the division                       -> rel_c = (rel_n + 2 u) / (1 - rel_n - u)
#   scale = min(1, c): exactly 1 when c (1 - rel_c) >= 1
# ---------------------------------------------------------------------------------------------------------------------------------
def clip_ref(g, max_norm, hyper=w):
    norm = float(np.sqrt((f64(g) ** 2).sum()))
    c = hyper(max_norm) / (norm + hyper(1e-6))
    return min(1.0, c), norm


def clip_bar(g, max_norm):
    n = np.asarray(g).size
    _, norm = clip_ref(g, max_norm)
    c = w(max_norm) / (norm + w(1e-6))
    rel_n = gam(n) / (2 - gam(n))
    rel_n = rel_n + U * (1 + rel_n)
    rel_c = (rel_n + 2 * U) / (1 - rel_n - U)
    return (0.0 if c * (1 - rel_c) >= 1 else rel_c * c), rel_n * norm


CLIP_WRONG = ("no_1e-6", "no_clamp")


def _block_sum(acc):
    """[blocks, 256] -> [blocks]: wave trees, then the waves in order"""
    wv = _wave_sum(acc.reshape(acc.shape[0], 4, 64))
    t = np.zeros(acc.shape[0], F)
    for k in range(4):
        t = t + wv[:, k]
    return t


def clip_f32(g, max_norm, wrong=None):
    g = np.asarray(g, F)
    n = g.size
    nb = min(1024, (n + 255) // 256)
    T = nb * 256
    pad = np.zeros((-n) % T, F)                   # a thread past the end adds nothing: x + 0 is exact
    sq = np.concatenate([g, pad]).reshape(-1, T)
    acc = np.zeros(T, F)
    for trip in sq:
        acc = acc + trip * trip
    partial = _block_sum(acc.reshape(nb, 256))
    acc = np.zeros(256, F)
    for trip in np.concatenate([partial, np.zeros((-nb) % 256, F)]).reshape(-1, 256):
        acc = acc + trip
    norm = np.sqrt(_block_sum(acc[None, :])[0])
    c = F(max_norm) / (norm if wrong == "no_1e-6" else norm + F(1e-6))
    return (c if (c < ONE or wrong == "no_clamp") else ONE), norm


CLIP_SIZES = (1, 255, 262144 + 77)                 # the last: above the grid cap (1024 blocks x 256 threads)


def clip_cases(rng, n):
    """(name, g, max_norm): a norm far above max_norm, one below it (scale exactly 1), and a norm of 2e-6 against 1e-6"""
    g = spread(rng, n, -12, 3)
    norm = float(np.sqrt((f64(g) ** 2).sum()))
    tiny = (g * F(2e-6 / norm)).astype(F)
    return [("far above", g, 1e-3 * norm), ("below", g, 4.0 * norm + 1.0), ("tiny norm", tiny, 1e-6)]


# ---------------------------------------------------------------------------------------------------------------------------------
# colsum (two-stage): T = M (+ 1 with accumulate) terms in a fixed but unspecified order -> gam(T - 1) sum |x|
# ---------------------------------------------------------------------------------------------------------------------------------
def colsum_ref(a, out_old, accumulate):
    s = f64(a).sum(0)
    return s + f64(out_old) if accumulate else s


def colsum_bar(a, out_old, accumulate):
    s = np.abs(f64(a)).sum(0)
    terms = np.asarray(a).shape[0] + (1 if accumulate else 0)
    return gam(terms - 1) * (s + np.abs(f64(out_old)) if accumulate else s)


COLSUM_WRONG = ("no_accumulate", "ld_is_N")


def colsum_f32(flat, M, N, ld, out_old, accumulate, wrong=None):
    """flat: the floats from a[0][0] on, row stride ld"""
    flat = np.asarray(flat, F)
    if wrong == "ld_is_N":
        ld = N
    a = np.lib.stride_tricks.as_strided(flat, (M, N), (4 * ld, 4))
    R = min(64, max(1, (M + 255) // 256))
    rows_per = (M + R - 1) // R
    partial = np.zeros((R, N), F)
    for y in range(R):
        r0, r1 = y * rows_per, min(M, (y + 1) * rows_per)
        sh = []
        for wv in range(4):
            acc = np.zeros(N, F)
            for r in range(r0 + wv, r1, 4):
                acc = acc + a[r]
            sh.append(acc)
        partial[y] = (sh[0] + sh[1]) + (sh[2] + sh[3])
    acc = np.zeros(N, F)
    for y in range(R):
        acc = acc + partial[y]
    return np.asarray(out_old, F) + acc if (accumulate and wrong != "no_accumulate") else acc


COLSUM_SHAPES = ((1, 1, 1), (5, 20, 24), (257, 136, 136), (16385 + 300, 70, 72))   # the last: above 64 row groups of 256


def colsum_inputs(rng, M, N):
    a = (rng.standard_normal((M, N)) * 2.0 ** rng.integers(-20, 21, (1, N))).astype(F)
    return a, spread(rng, N, -20, 20)


# ---------------------------------------------------------------------------------------------------------------------------------
# relu_bwd: dz = r > 0 ? dr scale : 0.  One rounding; the zero pattern is exact (a positive denormal is positive, -0.0 is not).
# ---------------------------------------------------------------------------------------------------------------------------------
def relu_bwd_ref(dr, r, scale, hyper=w):
    with np.errstate(invalid="ignore"):
        return np.where(np.asarray(r) > 0, f64(dr) * hyper(scale), 0.0)


def relu_bwd_bar(dr, r, scale):
    return U * np.abs(relu_bwd_ref(dr, r, scale))


RELU_WRONG = ("ge", "no_scale")


def relu_bwd_f32(dr, r, scale, wrong=None):
    r, dr = np.asarray(r, F), np.asarray(dr, F)
    keep = r >= 0 if wrong == "ge" else r > 0
    with np.errstate(invalid="ignore"):
        return np.where(keep, dr if wrong == "no_scale" else dr * F(scale), F(0))


RELU_SIZES = (4, 1028, 4194304 + 1024)             # the last: above the grid cap (4096 blocks x 256 threads x 4)


def relu_inputs(rng, n):
    """r holds 0, -0.0, a positive denormal and negatives; dr holds NaN wherever r <= 0"""
    r = spread(rng, n, -10, 3)
    special = np.array([0.0, -0.0, DENORM, -1.5], F)
    for k in range(4):
        r[k::max(4, n // 3)][:3] = special[k]
    if n > 4:
        r[n - 1] = 0.0
    dr = spread(rng, n, -10, 10)
    dr[~(r > 0)] = np.nan
    return dr, r


# ---------------------------------------------------------------------------------------------------------------------------------
# first_nonfinite: exact.  (first segment holding a NaN / Inf or 0x7fffffff, number of non-finite elements)
# ---------------------------------------------------------------------------------------------------------------------------------
def first_nonfinite_ref(buf, seg_start):
    bad = np.flatnonzero(~np.isfinite(np.asarray(buf, F)))
    if bad.size == 0:
        return NO_SEGMENT, 0
    return int(np.searchsorted(np.asarray(seg_start), bad[0], side="right") - 1), int(bad.size)


NONFINITE_WRONG = ("nan_only", "off_by_one")


def first_nonfinite_f32(buf, seg_start, wrong=None):
    """the kernel's bit test and binary search"""
    buf = np.ascontiguousarray(buf, F)
    bits = buf.view(np.uint32)
    hit = np.isnan(buf) if wrong == "nan_only" else (bits & np.uint32(0x7F800000)) == np.uint32(0x7F800000)
    first = NO_SEGMENT
    for e in np.flatnonzero(hit):
        lo, hi = 0, len(seg_start) - 1
        while lo < hi:
            mid = (lo + hi + 1) >> 1
            if (seg_start[mid] < e if wrong == "off_by_one" else seg_start[mid] <= e):
                lo = mid
            else:
                hi = mid - 1
        first = min(first, lo)
    return first, int(hit.sum())


NONFINITE_SIZES = (1, 6, 2097152 + 5)              # the last: above the grid cap (2048 blocks x 256 threads x 4), partial last quad


def nonfinite_segments(n):
    """five ascending segment starts, one segment of length 1.  n = 1 cannot hold five segments: its starts 1 .. 4 lie past the
    buffer (legal: the kernel only compares element indices with them)"""
    if n <= 6:
        return np.array([0, 1, 2, 4, 5] if n == 6 else [0, 1, 2, 3, 4], np.int64)
    return np.array([0, 1, n // 3, n // 3 + 1021, n - 2], np.int64)       # lengths 1, .., .., .., 2 (the tail quad is in the last two)


def nonfinite_base(rng, n):
    buf = spread(rng, n, -10, 10)
    buf[0::5] = DENORM
    buf[1::7] = FLT_MAX
    buf[2::11] = -FLT_MAX
    buf[3::13] = -DENORM
    return buf


def nonfinite_placements(n, seg):
    """lists of element indices: none; the first and last element of a segment; the tail quad; two segments at once"""
    if n == 1:
        return [[], [0]]
    s2, s3 = int(seg[2]), int(seg[3])
    tail = (n - 1) // 4 * 4
    out = [[], [s2], [s3 - 1], [0], [n - 1], [tail], [s2, n - 1], [s3 - 1, s3]]
    if n > 4096:
        out.append([s3 + 5, 5 * 1024 + 1, n - 3])           # three different workgroups, two segments
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# packed_row_index: exact.  idx[r] = b L + (r - cu[b]) for cu[b] <= r < cu[b + 1]
# ---------------------------------------------------------------------------------------------------------------------------------
def packed_row_index_ref(cu, L):
    cu = np.asarray(cu, np.int64)
    out = [b * L + j for b in range(len(cu) - 1) for j in range(int(cu[b + 1] - cu[b]))]
    return np.array(out, np.int32)


def packed_row_index_f32(cu, L):
    """the kernel's binary search over the prefix sums"""
    B, n = len(cu) - 1, int(cu[-1])
    idx = np.zeros(n, np.int32)
    for r in range(n):
        lo, hi = 0, B
        while hi - lo > 1:
            mid = (lo + hi) >> 1
            if cu[mid] <= r:
                lo = mid
            else:
                hi = mid
        idx[r] = lo * L + (r - cu[lo])
    return idx


PACKED_LENGTHS = ([0, 3, 0, 0, 5, 1, 0], [7], [0], [0, 0, 300, 0, 17, 0])     # empty slates first, in the middle, last; B == 1; n == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# nn.LayerNorm forward (ltrx_layernorm_torch_fwd_kernel), per row of D
#   mean^ = fl(S / D), S any-order over D terms: D - 1 additions and the division       -> bar_mean = gam(D) mean(|x|)
#   d_c   = fl(x_c - mean^):  |d_c - xc_c| <= e_c = bar_mean + u (|xc_c| + bar_mean)       (xc = x - mean: the mean's rounding shifts
#           every entry of the row alike, which is what a row with |mean| >> std feels)
#   q     = var + eps from the d_c: the shift gives a = mean(2 |xc| e + e^2); the squares, D - 1 additions, the division by D and
#           the addition of eps give gam(D + 2) (var + a + eps)                          -> E_q = a + gam(D + 2) (var + a + eps)
#   r     = 1 / sqrt(q): mean value theorem, |q^-1/2 - q^^-1/2| <= E_q / 2 (q - E_q)^-3/2; the sqrt and the division 2 more
#                                                                                       -> bar_rstd = E_q / 2 (q - E_q)^-3/2 + gam(2) r (1 + ..)
#   y_c   = fl(fl(fl(d_c r^) w_c) + b_c): the propagated |w| (e_c (r + bar_rstd) + |xc_c| bar_rstd) and three roundings on
#           |w| (|xc_c| + e_c) (r + bar_rstd) + |b_c|
# ---------------------------------------------------------------------------------------------------------------------------------
def ln_ref(x, wt, b, eps, hyper=w):
    y, (xhat, r) = MO.torch_ln_fwd(f64(x), f64(wt), f64(b), hyper(eps))
    return y, f64(x).mean(-1), r[:, 0]


def ln_bar(x, wt, b, eps):
    x, wt, b, eps = f64(x), f64(wt), f64(b), w(eps)
    D = x.shape[1]
    mean = x.mean(-1, keepdims=True)
    bar_mean = gam(D) * np.abs(x).mean(-1, keepdims=True)
    xc = np.abs(x - mean)
    e = bar_mean + U * (xc + bar_mean)
    var = (xc * xc).mean(-1, keepdims=True)
    a = (2 * xc * e + e * e).mean(-1, keepdims=True)
    q = var + eps
    E_q = a + gam(D + 2) * (var + a + eps)
    assert (E_q < 0.5 * q).all()
    r = q ** -0.5
    bar_r = 0.5 * E_q * (q - E_q) ** -1.5
    bar_r = bar_r + gam(2) * (r + bar_r)
    bar_y = np.abs(wt) * (e * (r + bar_r) + xc * bar_r) + gam(3) * (np.abs(wt) * (xc + e) * (r + bar_r) + np.abs(b))
    return bar_y, bar_mean[:, 0], bar_r[:, 0]


LN_WRONG = ("unbiased", "eps_outside")


def _lane_sums(v):
    """[rows, D] -> [rows]: lane l adds columns l, l + 64, .. in order, then the wave tree"""
    rows, D = v.shape
    pad = np.concatenate([v, np.zeros((rows, (-D) % 64), F)], 1).reshape(rows, -1, 64)
    acc = np.zeros((rows, 64), F)
    for k in range(pad.shape[1]):
        acc = acc + pad[:, k]
    return _wave_sum(acc)


def ln_f32(x, wt, b, eps, wrong=None):
    x, wt, b = np.asarray(x, F), np.asarray(wt, F), np.asarray(b, F)
    D = x.shape[1]
    mean = _lane_sums(x) / F(D)
    d = x - mean[:, None]
    var = _lane_sums(d * d) / F(D - 1 if wrong == "unbiased" else D)
    r = ONE / (np.sqrt(var) + F(eps)) if wrong == "eps_outside" else ONE / np.sqrt(var + F(eps))
    return d * r[:, None] * wt + b, mean, r


LN_SHAPES = ((1, 1), (5, 20), (37, 136), (8192 + 7, 64))        # the last: above the grid cap (2048 blocks x 4 rows)


def ln_inputs(rng, rows, D):
    """row 1 is constant (variance 0) and row 2 has |mean| / std of about 1e4 (where there are that many rows)"""
    x = (rng.standard_normal((rows, D)) * 2 + 0.3).astype(F)
    if rows > 2:
        x[1] = F(0.7)
        x[2] = (1e4 + rng.standard_normal(D)).astype(F)
    wt = (1 + 0.1 * rng.standard_normal(D)).astype(F)
    b = (0.1 * rng.standard_normal(D)).astype(F)
    gy = spread(rng, rows * D, -4, 4).reshape(rows, D)
    return x, wt, b, gy


# the parameter gradients of ltrx_layernorm_bwd called with the statistics the forward saved: xhat = (x - mean) rstd with THOSE fp32
# statistics;  dw = sum_rows gy xhat: the subtraction, two products and rows - 1 additions -> gam(rows + 2) sum |gy xhat|;
# db = sum_rows gy -> gam(rows - 1) sum |gy|
def ln_grad_ref(x, mean, rstd, wt, gy):
    xhat = (f64(x) - f64(mean)[:, None]) * f64(rstd)[:, None]
    grads = {}
    MO.torch_ln_bwd((xhat, f64(rstd)[:, None]), f64(wt), f64(gy), grads, "n")
    return grads["n.weight"], grads["n.bias"]


def ln_grad_bar(x, mean, rstd, gy):
    rows = np.asarray(x).shape[0]
    xhat = (f64(x) - f64(mean)[:, None]) * f64(rstd)[:, None]
    return gam(rows + 2) * np.abs(f64(gy) * xhat).sum(0), gam(rows - 1) * np.abs(f64(gy)).sum(0)


def ln_grad_f32(x, mean, rstd, gy):
    x, gy = np.asarray(x, F), np.asarray(gy, F)
    xhat = (x - np.asarray(mean, F)[:, None]) * np.asarray(rstd, F)[:, None]
    t = gy * xhat
    dw, db = np.zeros(x.shape[1], F), np.zeros(x.shape[1], F)
    for r in range(x.shape[0]):
        dw, db = dw + t[r], db + gy[r]
    return dw, db


# ---------------------------------------------------------------------------------------------------------------------------------
# positional encoding.  row(m) = padding_idx for a masked item and for a rank outside [0, padding_idx], else the rank (exact).
#   forward  y = scale x + table[row]: a product and an addition                          -> gam(2) (|scale x| + |table[row]|)
#   table gradient  dtable[r] = sum of dx[m] over row(m) == r < padding_idx, h terms       -> gam(h - 1) sum |dx[m]|; the padding row
#   is exactly 0, and so is a row that no item selects
# ---------------------------------------------------------------------------------------------------------------------------------
def posenc_rows(indices, mask, pad):
    i = np.asarray(indices, np.int64)
    rows = np.where((i < 0) | (i > pad), pad, i)
    if mask is not None:
        rows = np.where(np.asarray(mask) != 0, pad, rows)
    return rows.astype(np.int64)


def posenc_ref(x, table, indices, mask, pad, scale, hyper=w):
    return hyper(scale) * f64(x) + f64(table)[posenc_rows(indices, mask, pad)]


def posenc_bar(x, table, indices, mask, pad, scale):
    return gam(2) * (np.abs(w(scale) * f64(x)) + np.abs(f64(table)[posenc_rows(indices, mask, pad)]))


POSENC_WRONG = ("no_mask", "scale_table")


def posenc_f32(x, table, indices, mask, pad, scale, wrong=None):
    rows = posenc_rows(indices, None if wrong == "no_mask" else mask, pad)
    t = np.asarray(table, F)[rows]
    x = np.asarray(x, F)
    return F(scale) * (x + t) if wrong == "scale_table" else F(scale) * x + t


def posenc_table_bwd_ref(dx, indices, mask, pad):
    rows = posenc_rows(indices, mask, pad)
    out = np.zeros((pad + 1, np.asarray(dx).shape[1]), np.float64)
    np.add.at(out, rows, f64(dx))
    out[pad] = 0.0
    return out


def posenc_table_bwd_bar(dx, indices, mask, pad):
    rows = posenc_rows(indices, mask, pad)
    s = np.zeros((pad + 1, np.asarray(dx).shape[1]), np.float64)
    np.add.at(s, rows, np.abs(f64(dx)))
    hits = np.bincount(rows, minlength=pad + 1)
    bar = gam(np.maximum(hits - 1, 0))[:, None] * s
    bar[pad] = 0.0
    return bar


POSENC_BWD_WRONG = ("no_mask", "pad_row")


def posenc_table_bwd_f32(dx, indices, mask, pad, wrong=None):
    """a table row's four waves take the items 64 at a time (wave v: items 64 v + 256 k ..), ascending, then (0 + 1) + (2 + 3)"""
    dx = np.asarray(dx, F)
    M, D = dx.shape
    rows = posenc_rows(indices, None if wrong == "no_mask" else mask, pad)
    out = np.zeros((pad + 1, D), F)
    wave = (np.arange(M) // 64) % 4
    for r in range(pad + 1 if wrong == "pad_row" else pad):
        part = np.zeros((4, D), F)
        for m in np.flatnonzero(rows == r):
            part[wave[m]] = part[wave[m]] + dx[m]
        out[r] = (part[0] + part[1]) + (part[2] + part[3])
    return out


POSENC_SHAPES = ((7, 4, 3), (3 * 70, 20, 64), (2 * 300, 64, 240))      # (M, D, padding_idx); M D / 4 = 7, 1050, 9600


def posenc_inputs(rng, M, D, pad):
    """slates of M / (1, 3, 2) items whose ranks are a permutation of 0 .. L-1 (L - 1 > padding_idx: the long ranks fall on the padding
    row), then the edge ranks -1, padding_idx - 1, padding_idx, padding_idx + 1 and three above 2^31 whose low words are small"""
    nsl = {7: 1, 210: 3, 600: 2}[M]
    L = M // nsl
    idx = np.concatenate([rng.permutation(L) for _ in range(nsl)]).astype(np.int64)
    edge = [-1, pad - 1, pad, pad + 1, 2 ** 32 + 1, 2 ** 31 + 2, 2 ** 40]
    if M == 7:
        idx[:] = [-1, 2, 3, 4, 2 ** 32 + 1, 0, 2]              # rows 3 2 3 3 3 0 2: row 0 once, row 1 never, row 2 twice
    else:
        idx[L - len(edge):L] = edge
        idx[L + 3] = 1                                          # (and row 1 once more, from another slate)
        if nsl > 1:
            idx[idx == 5] = pad + 7                             # a row that nothing selects
    mask = (rng.random(M) < 0.15).astype(np.uint8)
    mask[0 if M == 7 else 11] = 1
    x = spread(rng, M * D, -8, 8).reshape(M, D)
    table = spread(rng, (pad + 1) * D, -8, 8).reshape(pad + 1, D)
    table[table == 0] = 1.0
    dx = spread(rng, M * D, -8, 8).reshape(M, D)
    return x, table, idx, mask, dx


# ---------------------------------------------------------------------------------------------------------------------------------
# scale_inplace: one rounding.   Output activations, kind 1 = sigmoid, 2 = tanh:
#   sigmoid y = 1 / (1 + expf(-z)): expf off by P u e relatively, the addition and the division -> (P + 2) u y + FLT_MIN (for z <
#           -87 the true value is below the normal range and expf overflows: the kernel may return 0)
#   tanh    y = tanhf(z)                                                                      -> P u |y| + FLT_MIN
#   backward from the saved y: sigmoid dz = dy (y (1 - y)): three roundings of one product  -> gam(3) |dz| + FLT_MIN
#           tanh dz = dy (1 - y y): u y^2 from the square, then the subtraction and the product -> |dy| (u y^2 + gam(2) |1 - y^2|) + FLT_MIN
# ---------------------------------------------------------------------------------------------------------------------------------
def scale_ref(x, s, hyper=w):
    return f64(x) * hyper(s)


def scale_bar(x, s):
    return U * np.abs(scale_ref(x, s))


def out_act_ref(z, kind):
    z = f64(z)
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-z)) if kind == 1 else np.tanh(z)


def out_act_bar(z, kind):
    y = np.abs(out_act_ref(z, kind))
    return ((P_LIBM + 2) if kind == 1 else P_LIBM) * U * y + FLT_MIN


def out_act_f32(z, kind):
    z = np.asarray(z, F)
    with np.errstate(over="ignore"):
        return ONE / (ONE + np.exp(-z)) if kind == 1 else np.tanh(z)


def out_act_bwd_ref(dy, y, kind):
    dy, y = f64(dy), f64(y)
    return dy * (y * (1 - y) if kind == 1 else 1 - y * y)


def out_act_bwd_bar(dy, y, kind):
    dy, y = np.abs(f64(dy)), f64(y)
    if kind == 1:
        return gam(3) * dy * np.abs(y * (1 - y)) + FLT_MIN
    return dy * (U * y * y + gam(2) * np.abs(1 - y * y)) + FLT_MIN


OUT_ACT_BWD_WRONG = ("at_z",)


def out_act_bwd_f32(dy, y, kind, z=None, wrong=None):
    dy, v = np.asarray(dy, F), np.asarray(z if wrong == "at_z" else y, F)
    return dy * (v * (ONE - v) if kind == 1 else ONE - v * v)


def out_act_inputs(rng):
    edge = np.array([0, 1e-8, 1, 20, 100], F)
    z = np.concatenate([edge, -edge, spread(rng, 300, -6, 3)]).astype(F)
    return z, spread(rng, z.size, -6, 6)
