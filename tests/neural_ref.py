"""fp64 references, entrywise bars, fp32 transcriptions and the case table of the NeuralNDCG kernels (allrank_amd/csrc/ltrx_neuralndcg.hip:
the ideal-DCG prologue, the general forward / backward kernels, the four block-resident geometries, the residual and pick-iteration
kernels)  --  TEST INFRASTRUCTURE, plain numpy, needs no GPU.  The machinery (F, U, w, worst, over, PAD, P_HW) is tests/listwise_ref.py's.

    neural_ref     allrank/models/losses/neuralNDCG.py and loss_utils.py as read, in fp64: the L x L MASKED formulation (padded rows and
                   columns stay in the matrices: -1e8 scores, the -inf / 1 fills, the 0 / 1 fills of sinkhorn_scaling, the masks behind it),
                   NOT the kernel's compacted valid block.  scaling_i goes by the row's position in the uncompacted slate (loss_utils.py:
                   54-57).  The plain read-out (neuralNDCG.py:46-63) and the transposed one (:110-129: expected discounts, RAW labels as
                   gains, an ideal DCG that is always powered) are separate code paths.  It returns loss, per-slate values, gradient,
                   idcg [B], the nonzero count, the residual trace res[b][it] and T*, and per entry the magnitude `cond` of its bar.
                   `k_rows` caps the ranks that carry a discount per slate (min(k, k_rows[b])), as the ABI documents.
    _core          the same code in any dtype and summation order: with np.float32 and the orders of ORDERS it is the fp32 transcription of
                   the REFERENCE formulation (states of every step stored, adjoint (g - d) / c by stored states) that K is measured with.
    neural_f32     the kernels' operation order in np.float32: compaction, two-pass softmax with the rounded z, column step then row step
                   with normalisers clamped at 1e-10 and kept, all max_iter steps run, the state rewound by (S * r) * c from max_iter to
                   T*, the adjoint Xbar = (Ybar - [c > 1e-10] sum(Ybar Y)) / c with the state recovered as Y * c; ``wrong=`` defect models.

The exit step.  T* = the first step at which the batch maximum residual is below tol (loss_utils.py:25), else max_iter.  fp32 and fp64
residuals differ, so every case that wants an early exit at step T derives its tol from the fp64 trace m[it] = max_b res[b][it]: tol =
sqrt(m[T - 2] m[T - 1]) (T counts steps run: m[T - 1] is the residual after the T-th step).  The case is admitted only if m[it] - tol >=
GUARD * resbar for every step before the T-th and tol - m[T - 1] >= GUARD * resbar, where resbar = (n + 2 T + Zmax) u is the fp32 error bar
of a residual: a column sum of n terms near 1 (n u), a state that has gone through 2 T divisions (2 T u) and whose exponent arguments
carry Zmax u (below); and tol >= GUARD * n u, the fp32 noise floor of a row / column sum.  tests/test_neural_ref_cpu.py checks that the
fp32 transcriptions pick the same T* on every such case.  A wanted T* that cannot be guarded is a reason to change the inputs.

Bars.  bar = K u cond + floor for every gradient entry, per-slate value, idcg entry and the loss.  cond is computed by the fp64 reference:
    Zmax      max over the valid block of (|scaling_i s_j| + Bsum_j) / tau: the absolute error of the exponent argument of P0 in units of u
              -- it grows with |s|, n and 1 / tau.  Softmax and Sinkhorn are scale invariant per row and column and every step
              renormalises, so an entry of the state carries a relative error of the order (W_STATE + Zmax) u whatever the step: the
              perturbation of P0 is ONE perturbation, it is counted once (at the seed of the reverse pass and in the softmax Jacobian), and
              a step adds its own W_STATE roundings
    value_b   a sum of non-negative terms disc_i P_ij g_j: cond = value_b (W_STATE + Zmax + 8)   (idcg, the division, the gains)
    idcg_b    a sum of non-negative terms: cond = idcg_b;    loss: sum_b cond(value_b) / count
    gradient  an absolute-value reverse pass, seeded with (4 + Zmax) |Ybar|.  At every reversed half step Y = X / c the entry Xbar = (Ybar -
              d) / c, d = [c > eps] sum Ybar Y, is formed from the terms |Ybar| and sum |Ybar| Y (weighted 3 + W_STATE: the dot's roundings
              and the state's); their sum is carried along divided by the same normalisers, E <- (E + |Ybar| + (3 + W_STATE) sum |Ybar| Y) /
              c, with the signed Ybar of that step.  E is NOT fed through d again: g -> g - <g, y> removes a row's (column's) common part,
              it does not amplify, and a worst-case running bound through 2 x 50 such steps doubles per step and says nothing.  The softmax
              Jacobian P0 (g0 - <g0, P0>) / tau adds P0 (E0 + <E0, P0> + (4 + Zmax) (|g0| + <|g0|, P0>)) / tau, and the last stage sums
              these magnitudes with |scaling_i| and the signs of s_j - s_m as the gradient itself is summed.
    floor     FLT_MIN n^2 max(1, 1 / tau): an exponential below FLT_MIN has no relative precision in fp32.
K is measured, not derived: the worst |fp32 - fp64| / (u cond) per output over the whole case table of _core(np.float32) in the three
summation orders of ORDERS (numpy's pairwise one, strictly sequential, and the four contiguous partials ((p0 + p1) + p2) + p3 of
LTRX_PART4); K = FACTOR x that worst, FACTOR = 4: numpy rounds exp and the divisions correctly where the device's expf and division are
allowed 2 ulp (P_HW), and the five kernel geometries sum in five more orders.  `measure()` recomputes WORST; the kernel's own worst error /
bar is only ever logged and never feeds back.

What the bars do not see.  cond is a sum of magnitudes, so an entry that is the small remainder of large cancelling terms (the tail of a
long slate) has a bar far above its own size, and Zmax is a worst case that a saturated P0 does not realise: at score scale 30 and at tau =
0.1 with n > 100 the gradient bars reach the size of the largest entry of the slate (the fp32 transcriptions sit at 1e-5 .. 1e-4 of them),
and only the per-slate values (bars of 1e-3 relative and less), the exact outputs and the zero pattern bind there.  The bars bind where the
defect models are named: bar / |entry| has a median of 1e-4 at n = 3, 7e-4 at 65 items and tau = 10, 7e-3 .. 2e-2 at 64 items.  Every tile
geometry therefore also has a slate of one tile plus one item.

Guards (conditions on the inputs, asserted by neural_ref): no normaliser within 1 % of the clamp 1e-10, and a clamped one above 1e-30 (a
column that underflows in fp32 stays clamped for ever where fp64 leaves the clamp after a few steps: the reference's own fp32 behaviour,
reached only with interior pads at large score scale, and outside any fp32-vs-fp64 comparison).
"""
import functools
from collections import namedtuple

import numpy as np

from tests.listwise_ref import F, FLT_MIN, PAD, U, f64, over, w, worst  # noqa: F401  (re-exported)

SINK_EPS = w(1e-10)              # DEFAULT_EPS as the fp32 kernels (and torch's fp32 clamp) see it
GUARD = 4.0
W_STATE = 4.0                    # roundings an entry of a Sinkhorn state carries whatever the step (see Bars)
FACTOR = 4.0
ORDERS = ("numpy", "sequential", "part4")
# measured by measure() over CASES x ORDERS (worst |fp32 - fp64| / (u cond), rounded up), the factor, and K = FACTOR x WORST
WORST = dict(grad=0.087, per=0.19, loss=0.12, idcg=5.7)
K = {k_: FACTOR * v for k_, v in WORST.items()}

# restated from ltrx_neuralndcg.hip; tests/test_neural_ref_cpu.py holds them to the text
BLOCK_MAX_L = 240
GEOMETRIES = ((64, "blk 2x2", 2), (128, "blk 4x4", 4), (192, "blk 6x6", 6), (240, "blk 15x5", 5))       # (largest L, arm, tile width)
MAX_SLATE_LEN = 2048
EXPECTED_ARMS = {(0, 64): "blk 2x2", (0, 65): "blk 4x4", (0, 128): "blk 4x4", (0, 129): "blk 6x6", (0, 192): "blk 6x6", (0, 193): "blk 15x5",
                 (0, 240): "blk 15x5", (0, 241): "general", (1, 64): "general", (1, 240): "general"}


def arm_of(path, L):
    if path == 0:
        for top, arm, _ in GEOMETRIES:
            if L <= top:
                return arm
    return "general"


def tile_width(L):
    for top, _, wd in GEOMETRIES:
        if L <= top:
            return wd
    return None


def align64(x):
    return (x + 63) & ~63


def workspace_bytes(B, L, max_iter):
    """ltrx_neuralndcg_workspace_bytes restated: per [B], res [B][mi], titer, cn [B][mi + 1][L], rn [B][mi][L], S and A [B][L][L], 64 spare"""
    mi = max(max_iter, 1)
    return (align64(B * 4) + align64(B * mi * 4) + 64 + align64(B * (mi + 1) * L * 4) + align64(B * mi * L * 4) + 2 * align64(B * L * L * 4) + 64)


# ---------------------------------------------------------------------------------------------------------------------------------
# summation orders
# ---------------------------------------------------------------------------------------------------------------------------------
class Sums(object):
    def __init__(self, dt, order="numpy"):
        self.dt, self.order = dt, order

    def _seq(self, M):
        acc = np.zeros(M.shape[0], self.dt)
        for j in range(M.shape[1]):
            acc = acc + M[:, j]
        return acc

    def ax(self, M, axis):
        """the sum of a matrix over `axis`"""
        M = M if axis == 1 else M.T
        if self.order == "numpy":
            return M.sum(axis=1, dtype=self.dt)
        if self.order == "sequential":
            return self._seq(M)
        q = max(1, -(-M.shape[1] // 4))
        p = [self._seq(M[:, a * q:(a + 1) * q]) for a in range(4)]
        return ((p[0] + p[1]) + p[2]) + p[3]

    def vec(self, v):
        return self.ax(np.asarray(v, self.dt)[None, :], 1)[0]


Par = namedtuple("Par", "tau powered k k_rows transposed max_iter")      # k <= 0: none; k_rows: None or one int per slate


def _kk(k, L):
    return L if (k <= 0 or k > L) else k


def _gain(t, powered, dt):
    return (np.exp2(t).astype(dt) - dt(1)) if powered else t.astype(dt)


def ideal_dcg(y, k, powered, dt, S, padded_gain_kept=False):
    """metrics.dcg(y_true, y_true, ats=[k]) of one slate (metrics.py:32-75): padded labels become 0 and sort last"""
    mask = y == PAD
    t = np.where(mask, dt(0), y).astype(dt)
    key = np.where(mask, -np.inf, f64(y))
    order = np.argsort(-key, kind="stable")
    tsp = (y.astype(dt) if padded_gain_kept else t)[order]
    disc = (dt(1) / np.log2(np.arange(len(y)).astype(dt) + dt(2))).astype(dt)
    return S.vec((_gain(tsp, powered, dt) * disc)[:_kk(k, len(y))])


def _neural_sort(s, mask, tau, dt, S):
    """deterministic_neural_sort of one slate (loss_utils.py:46-66): (P_hat [L, L], scaling [L], Zmax)"""
    L = len(s)
    n = int(L - mask.sum())
    either, both = mask[:, None] | mask[None, :], mask[:, None] & mask[None, :]
    sm = np.where(mask, dt(-1e8), s).astype(dt)
    A = np.where(either, dt(0), np.abs(sm[:, None] - sm[None, :])).astype(dt)
    Bsum = S.ax(A, 1)
    i = np.arange(L)
    scaling = np.where(i < n, n + 1 - 2 * (i + 1), 0).astype(dt)
    s0 = np.where(mask, dt(0), s).astype(dt)
    C = (scaling[:, None] * s0[None, :]).astype(dt)
    P_max = (C - Bsum[None, :]).astype(dt)
    P_max = np.where(either, dt(-np.inf), P_max)
    P_max = np.where(both, dt(1), P_max).astype(dt)
    z = (P_max / dt(tau)).astype(dt)
    with np.errstate(under="ignore"):
        e = np.exp((z - z.max(axis=1, keepdims=True)).astype(dt)).astype(dt)
    P = (e / S.ax(e, 1)[:, None]).astype(dt)
    valid = ~either
    zmax = float(((np.abs(f64(C)) + f64(Bsum)[None, :]) / float(tau))[valid].max()) if valid.any() else 0.0
    return P, scaling, zmax


def _sinkhorn(P_hat, mask, steps, dt, S, keep):
    """sinkhorn_scaling of one slate without its exit (loss_utils.py:17-23): `steps` steps; (masked output, res [steps], the (c, r, y1,
    y2, unclamped c, unclamped r) of the first `keep` steps, the output after `keep` steps)"""
    eps = dt(SINK_EPS)
    either, both = mask[:, None] | mask[None, :], mask[:, None] & mask[None, :]
    mat = np.where(either, dt(0), P_hat)
    mat = np.where(both, dt(1), mat).astype(dt)
    res, states, at_keep = np.zeros(steps), [], mat
    with np.errstate(under="ignore"):
        for it in range(steps):
            c0 = S.ax(mat, 0)
            c = np.maximum(c0, eps)
            y1 = (mat / c[None, :]).astype(dt)
            r0 = S.ax(y1, 1)
            r = np.maximum(r0, eps)
            y2 = (y1 / r[:, None]).astype(dt)
            res[it] = max(float(np.abs(S.ax(y2, 1) - dt(1)).max()), float(np.abs(S.ax(y2, 0) - dt(1)).max()))
            if it < keep:
                states.append((c, r, y1, y2, c0, r0))
            mat = y2
            if it + 1 == keep:
                at_keep = mat
    return res, states, np.where(either, dt(0), at_keep).astype(dt)


def exit_step(res, tol, max_iter):
    """T*: res [B, max_iter]"""
    m = res.max(axis=0) if res.shape[0] else np.zeros(max_iter)
    for it in range(max_iter):
        if m[it] < tol:
            return it + 1
    return max_iter


def _core(s, y, p, tol, dt=np.float64, order="numpy", cond=False, idcg_given=None):
    """the reference formulation over a batch in dtype dt and one summation order"""
    S = Sums(dt, order)
    s, y = np.asarray(s, F).astype(dt), np.asarray(y, F)
    B, L = s.shape
    masks = y == PAD
    idcg_powered = bool(p.powered or p.transposed)                      # neuralNDCG.py:55-58 vs :121 / :125
    idcg = np.array([ideal_dcg(y[b], p.k, idcg_powered, dt, S) for b in range(B)], dt) if idcg_given is None else np.asarray(idcg_given, dt)
    zero = idcg == 0
    cnt = int((~zero).sum())
    sorts = [_neural_sort(s[b], masks[b], p.tau, dt, S) for b in range(B)]
    res = np.stack([_sinkhorn(sorts[b][0], masks[b], p.max_iter, dt, S, 0)[0] for b in range(B)]) if B else np.zeros((0, p.max_iter))
    T = exit_step(res, tol, p.max_iter)
    disc = (dt(1) / np.log2(np.arange(L).astype(dt) + dt(2))).astype(dt)
    per, grads, c_per, c_grad, norm_min = np.zeros(B, dt), np.zeros((B, L), dt), np.zeros(B), np.zeros((B, L)), []
    for b in range(B):
        mask, (P_hat, scaling, zmax) = masks[b], sorts[b]
        either = mask[:, None] | mask[None, :]
        n = int(L - mask.sum())
        kk = _kk(p.k, L) if p.k_rows is None else min(_kk(p.k, L), int(p.k_rows[b]))
        disc_k = disc.copy()
        disc_k[kk:] = 0
        _, states, P_s = _sinkhorn(P_hat, mask, T, dt, S, T)
        for st in states:
            norm_min.append((st[4][~mask], st[5][~mask]))
        if p.transposed:
            g = _gain(y[b], p.powered, dt)                                                   # :119 / :123: raw labels
            exp_disc = S.ax((P_s * disc_k[:, None]).astype(dt), 0)                           # :117
            dgain = S.vec((g * exp_disc).astype(dt))                                         # :120 / :124, :127
        else:
            g = _gain(np.where(mask, dt(0), y[b]), p.powered, dt)                            # :47-49
            gt = S.ax((P_s * g[None, :]).astype(dt), 1)                                      # :51
            dgain = S.vec((gt * disc_k).astype(dt))                                          # :53, :60-61
        if zero[b]:
            continue                                                                         # :62-63: value 0, no gradient
        per[b] = dgain / (idcg[b] + dt(SINK_EPS))
        c_per[b] = float(per[b]) * (W_STATE + zmax + 8.0)
        if cnt == 0 or n == 0:
            continue
        coef = dt(-1.0) / (dt(cnt) * (idcg[b] + dt(SINK_EPS)))
        gb = np.where(either, dt(0), coef * disc_k[:, None] * g[None, :]).astype(dt)
        E = (4.0 + zmax) * np.abs(f64(gb)) if cond else None
        with np.errstate(under="ignore"):
            for t in range(T, 0, -1):
                c, r, y1, y2 = states[t - 1][:4]
                on = (r > dt(SINK_EPS))
                d = S.ax((gb * y2).astype(dt), 1) * on
                if cond:
                    E = (E + np.abs(f64(gb)) + (3.0 + W_STATE) * (np.abs(f64(gb)) * f64(y2)).sum(1, keepdims=True) * on[:, None]) / f64(r)[:, None]
                gb = ((gb - d[:, None]) / r[:, None]).astype(dt)
                on = (c > dt(SINK_EPS))
                d = S.ax((gb * y1).astype(dt), 0) * on
                if cond:
                    E = (E + np.abs(f64(gb)) + (3.0 + W_STATE) * (np.abs(f64(gb)) * f64(y1)).sum(0, keepdims=True) * on[None, :]) / f64(c)[None, :]
                gb = ((gb - d[None, :]) / c[None, :]).astype(dt)
            g0 = np.where(either, dt(0), gb).astype(dt)                                      # loss_utils.py:17-18 block the gradient
            inner = S.ax((g0 * P_hat).astype(dt), 1)
            gz = np.where(either, dt(0), P_hat * (g0 - inner[:, None]) / dt(p.tau)).astype(dt)
        grad = S.ax((gz * scaling[:, None]).astype(dt), 0)
        Q = S.ax(gz, 0)
        sm = np.where(mask, dt(0), s[b])
        sgn = np.where(either, dt(0), np.sign(sm[:, None] - sm[None, :])).astype(dt)         # sgn[j, m] = sign(s_j - s_m)
        grad = grad - Q * S.ax(sgn, 1) + S.ax((Q[:, None] * sgn).astype(dt), 0)
        grads[b] = np.where(mask, dt(0), grad)
        if cond:
            P64, E0, a0 = f64(P_hat), np.where(either, 0.0, E), np.abs(f64(g0))
            Ez = np.where(either, 0.0, P64 * (E0 + (E0 * P64).sum(1, keepdims=True) + (4.0 + zmax) * (a0 + (a0 * P64).sum(1, keepdims=True))) / float(p.tau))
            QE = Ez.sum(0)
            c_grad[b] = np.where(mask, 0.0, (Ez * np.abs(f64(scaling))[:, None]).sum(0) + QE * np.abs(f64(sgn).sum(1)) + (QE[:, None] * np.abs(f64(sgn))).sum(0))
    loss = dt(0) if cnt == 0 else -S.vec(per) / dt(cnt)                                      # :66-70
    out = dict(loss=loss, per=per, grad=grads, idcg=idcg, cnt=cnt, T=T, res=res, zero=masks | zero[:, None])
    if cond:
        nv = (~masks).sum(1)
        floor = FLT_MIN * max(1.0, 1.0 / p.tau)
        out.update(cond_per=c_per, cond_grad=c_grad, cond_idcg=np.abs(f64(idcg)), cond_loss=(c_per.sum() / cnt if cnt else 0.0),
                   floor_grad=(floor * nv * nv)[:, None] * np.ones((1, L)), floor_per=floor * nv * nv, zmax=np.array([t[2] for t in sorts]),
                   norm_min=norm_min)
    return out


def neural_ref(s, y, p, tol):
    ref = _core(s, y, p, tol, np.float64, "numpy", cond=True)
    for c, r in ref.pop("norm_min"):
        v = np.concatenate([c, r])
        assert (np.abs(v - SINK_EPS) > 0.01 * SINK_EPS).all() and (v > 1e-30).all(), "a normaliser is not clear of the clamp (or underflows in fp32)"
    return ref


def bars(ref):
    """{output: bar} = K u cond + floor"""
    return dict(grad=K["grad"] * U * ref["cond_grad"] + ref["floor_grad"], per=K["per"] * U * ref["cond_per"] + ref["floor_per"],
                loss=K["loss"] * U * ref["cond_loss"] + float(ref["floor_per"].sum()), idcg=K["idcg"] * U * ref["cond_idcg"])


def derive_tol(res, T, nmax, zmax):
    """(tol as the ABI receives it, admitted?) for an exit after T >= 2 steps, from the fp64 trace res [B, max_iter]"""
    m = res.max(axis=0)
    hi, lo = float(m[T - 2]), float(m[T - 1])
    tol = w(np.sqrt(hi * lo))
    resbar = (nmax + 2 * T + zmax) * U
    ok = (m[:T - 1] - tol >= GUARD * resbar).all() and tol - lo >= GUARD * resbar and tol >= GUARD * nmax * U
    return tol, bool(ok)


# ---------------------------------------------------------------------------------------------------------------------------------
# the kernels' operation order in fp32, with defect models
# ---------------------------------------------------------------------------------------------------------------------------------
WRONG = ("scaling_by_compacted_index", "per_slate_exit", "rewind_skipped", "clamp_adjoint_dropped", "row_step_before_column_step",
         "discount_k_inclusive", "k_rows_ignored", "tile_tail_column_dropped_2", "tile_tail_column_dropped_4", "tile_tail_column_dropped_6",
         "tile_tail_column_dropped_5", "idcg_gain_unpowered_in_transposed", "excluded_slate_counted", "gain_of_padded_not_zero",
         "residual_rows_only")


def neural_f32(s, y, p, tol, wrong=None):
    S = Sums(F)
    s, y = np.asarray(s, F), np.asarray(y, F)
    B, L = s.shape
    eps, one, tau, mi = F(SINK_EPS), F(1), F(p.tau), p.max_iter
    tail = int(wrong.rsplit("_", 1)[1]) if wrong and wrong.startswith("tile_tail") else 0
    idcg_powered = bool(p.powered or (p.transposed and wrong != "idcg_gain_unpowered_in_transposed"))
    idcg = np.array([ideal_dcg(y[b], p.k, idcg_powered, F, S, wrong == "gain_of_padded_not_zero") for b in range(B)], F)
    cnt = F(B) if wrong == "excluded_slate_counted" else F((idcg != 0).sum())
    inv_tau = F(one / tau)

    def rows(M, n):                                             # a row sum; the defect drops the columns of the last, partial tile
        return S.ax(M[:, :n - n % tail] if (tail and n > tail and n % tail) else M, 1)

    fw, res = [], np.zeros((B, mi))
    for b in range(B):
        vidx = np.flatnonzero(y[b] != PAD)
        n = len(vidx)
        if n == 0:
            fw.append(None)
            continue
        sc = s[b, vidx]
        Bs = np.abs(f64(sc)[:, None] - f64(sc)[None, :]).sum(1).astype(F)             # compensated: within an ulp of the exact sum
        scal = np.where(vidx < n, n + 1 - 2 * (vidx + 1), 0).astype(F)
        if wrong == "scaling_by_compacted_index":
            scal = (n + 1 - 2 * (np.arange(n) + 1)).astype(F)
        with np.errstate(under="ignore", divide="ignore", invalid="ignore"):
            z = (((scal[:, None] * sc[None, :]).astype(F) - Bs[None, :]).astype(F) / tau).astype(F)
            e = np.exp((z - z.max(1, keepdims=True)).astype(F)).astype(F)
            St = (e / rows(e, n)[:, None]).astype(F)
            cn, rn = np.zeros((mi, n), F), np.zeros((mi, n), F)
            for it in range(mi):
                if wrong == "row_step_before_column_step":
                    r = np.maximum(rows(St, n), eps)
                    St = (St / r[:, None]).astype(F)
                    c = np.maximum(S.ax(St, 0), eps)
                    St = (St / c[None, :]).astype(F)
                else:
                    c = np.maximum(S.ax(St, 0), eps)
                    St = (St / c[None, :]).astype(F)
                    r = np.maximum(rows(St, n), eps)
                    St = (St / r[:, None]).astype(F)
                cn[it], rn[it] = c, r
                rr = float(np.abs(rows(St, n) - one).max())
                res[b, it] = rr if wrong == "residual_rows_only" else max(rr, float(np.abs(S.ax(St, 0) - one).max()))
        fw.append((vidx, sc, scal, St, cn, rn))
    T = exit_step(res, F(tol), mi)
    per, grads = np.zeros(B, F), np.zeros((B, L), F)
    for b in range(B):
        if fw[b] is None or idcg[b] == 0:
            continue
        vidx, sc, scal, St, cn, rn = fw[b]
        n = len(vidx)
        Tb = T
        if wrong == "per_slate_exit":
            below = np.flatnonzero(res[b] < F(tol))
            Tb = int(below[0]) + 1 if len(below) else mi
        kk = _kk(p.k, L)
        if p.k_rows is not None and wrong != "k_rows_ignored":
            kk = min(kk, int(p.k_rows[b]))
        cut = (vidx <= kk) if wrong == "discount_k_inclusive" else (vidx < kk)
        dk = np.where(cut, one / np.log2(vidx.astype(F) + F(2)).astype(F), F(0)).astype(F)
        gc = _gain(y[b, vidx], p.powered, F)
        with np.errstate(under="ignore", over="ignore", invalid="ignore"):
            if wrong != "rewind_skipped":
                for it in range(mi - 1, Tb - 1, -1):
                    St = ((St * rn[it][:, None]).astype(F) * cn[it][None, :]).astype(F)
            a = S.ax((St * gc[None, :]).astype(F), 1)
            v = S.vec((dk * a).astype(F))
            per[b] = v / (idcg[b] + eps)
            coef = F(F(-1) / (cnt * (idcg[b] + eps)))
            A = ((coef * dk)[:, None] * gc[None, :]).astype(F)
            for it in range(Tb - 1, -1, -1):
                r, c = rn[it], cn[it]
                d = S.ax((A * St).astype(F), 1)
                d = np.where((r > eps) | (wrong == "clamp_adjoint_dropped"), d, F(0))
                A, St = ((A - d[:, None]) / r[:, None]).astype(F), (St * r[:, None]).astype(F)
                d = S.ax((A * St).astype(F), 0)
                d = np.where((c > eps) | (wrong == "clamp_adjoint_dropped"), d, F(0))
                A, St = ((A - d[None, :]) / c[None, :]).astype(F), (St * c[None, :]).astype(F)
            d = S.ax((A * St).astype(F), 1)
            gz = ((St * (A - d[:, None]).astype(F)).astype(F) * inv_tau).astype(F)
        direct, q = S.ax((gz * scal[:, None]).astype(F), 0), S.ax(gz, 0)
        sgn = np.sign(sc[:, None] - sc[None, :]).astype(F)
        grads[b, vidx] = (direct - (q * S.ax(sgn, 1)).astype(F)).astype(F) - S.ax((q[None, :] * sgn).astype(F), 1)
    loss = F(0) if cnt == 0 else F(-S.vec(per) / cnt)
    return dict(loss=loss, per=per, grad=grads, idcg=idcg, cnt=int(cnt), T=T, res=res)


# ---------------------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name L path counts pad zero scale ties tau powered k k_rows transposed max_iter T seed why")


def _cases():
    out = []

    def add(name, L, why, path=0, counts=None, pad="end", zero=(), scale=1, ties=None, tau=1.0, powered=True, k=0, k_rows=None, transposed=False,
            max_iter=50, T=None, seed=0):
        counts = tuple(counts if counts is not None else (L, max(L - 1, 0), 1, 0))
        out.append(Case("L %d path %d %s" % (L, path, name), L, path, counts, pad, tuple(zero), scale, ties, tau, powered, k, k_rows, transposed,
                        max_iter, T, seed, why))

    add("one item", 1, "n = 1 and n = 0 only: a softmax of one entry, a gradient of exactly 0")
    add("two items", 2, "the smallest slate with a gradient; k > n on the 1-item slate", k=5, counts=(2, 1, 2, 0), zero=(2,))
    add("base", 3, "the 3-item slates every older test uses, here against fp64", zero=(1,))
    add("general", 3, "the general kernels at the smallest length", path=1, powered=False)
    add("max_iter 0", 3, "no Sinkhorn step at all: the read-out and the adjoint of P0; T* = 0", max_iter=0)
    add("max_iter 1", 3, "one step: column step then row step is not row step then column step", max_iter=1, counts=(3, 3, 2, 0), seed=1)
    add("clamp", 6, "a leading pad: the row of the top scaling is missing, the far-off top item is nobody's first choice and its column sum 5.7e-11 is "
        "clamped at step 0 (the same items with the pad at the end beside it)", counts=(5, 5), pad="clamp", max_iter=3)
    add("all excluded", 3, "every slate all-zero or fully padded: count 0, loss 0, gradient 0", counts=(3, 0, 2), zero=(0, 2))
    add("interior pads k 5", 63, "2x2 tiles, n = 31 * 2 + 1; interior pads: valid rows at original index >= n", pad="inter", k=5, counts=(63, 62, 31, 1, 0))
    add("exit 4", 64, "rewind on the 2x2 tiles: 46 steps multiplied back", T=4, counts=(64, 63, 2, 33, 0))
    add("exit 4 general", 64, "rewind in the general kernels below 240; the same inputs as path 0", path=1, T=4, counts=(64, 63, 2, 33, 0))
    add("tau 10 linear gain", 65, "the first length of the 4x4 tiles; a flat P0", tau=10.0, powered=False, zero=(1,))
    add("exit 5 transposed", 128, "rewind on the 4x4 tiles, n = 31 * 4 + 1 and 4 + 1, the transposed formula with its powered idcg", T=5, transposed=True,
        powered=False, counts=(128, 127, 125, 5, 0))
    add("interior pads", 129, "the first length of the 6x6 tiles, interior pads", pad="inter", counts=(129, 128, 97, 1, 0))
    add("scale 30", 129, "the trained-model score scale: Zmax drives the bar", scale=30, counts=(129, 128, 1, 0))
    add("general scale 30", 129, "the general kernels at score scale", path=1, scale=30, counts=(129, 128, 1, 0))
    add("exit 4 k 1", 192, "rewind on the 6x6 tiles, n = 31 * 6 + 1 and 6 + 1, one discounted row", T=4, k=1, counts=(192, 191, 187, 7, 0))
    add("tau 0.1", 193, "the first length of the 15x5 tiles at a sharp P0", tau=0.1, counts=(193, 192, 1, 0), ties=1)
    add("exit 4 k_rows", 240, "rewind on the 15x5 tiles, n = 47 * 5 + 1 and 5 + 1, k_rows below k", T=4, k=20, k_rows=(7, 20, 3, 2, 5),
        counts=(240, 239, 236, 6, 0))
    add("general k_rows", 240, "the general kernels at the last block-resident length", path=1, k=20, k_rows=(7, 20, 3, 1), counts=(240, 239, 1, 0))
    add("exit 4", 241, "path 0 above 240 is the general kernel: its rewind", T=4, counts=(241, 240, 2, 0))
    add("batch-global exit", 64, "a 2-item slate is doubly stochastic at once, a 20-item one converges steps before the full one: T* is the batch's",
        T=6, counts=(2, 20, 64), seed=2)
    add("ties zero slate", 257, "the general kernel at two items per lane; quantised scores (exact ties); an all-zero slate", ties=0, zero=(1,),
        counts=(257, 256, 129, 0), transposed=True)
    return out


CASES = _cases()
REWIND_ARMS = ("blk 2x2", "blk 4x4", "blk 6x6", "blk 15x5", "general")
# the case on which each defect model must fall outside its bar
NAMED = {
    "scaling_by_compacted_index": "L 63 path 0 interior pads k 5",
    "per_slate_exit": "L 64 path 0 batch-global exit",
    "rewind_skipped": "L 64 path 0 exit 4",
    "clamp_adjoint_dropped": "L 6 path 0 clamp",
    "row_step_before_column_step": "L 3 path 0 max_iter 1",
    "discount_k_inclusive": "L 63 path 0 interior pads k 5",
    "k_rows_ignored": "L 240 path 0 exit 4 k_rows",
    "tile_tail_column_dropped_2": "L 63 path 0 interior pads k 5",
    "tile_tail_column_dropped_4": "L 128 path 0 exit 5 transposed",
    "tile_tail_column_dropped_6": "L 192 path 0 exit 4 k 1",
    "tile_tail_column_dropped_5": "L 240 path 0 exit 4 k_rows",
    "idcg_gain_unpowered_in_transposed": "L 128 path 0 exit 5 transposed",
    "excluded_slate_counted": "L 3 path 0 base",
    "gain_of_padded_not_zero": "L 3 path 0 base",
    "residual_rows_only": "L 64 path 0 exit 4",
}


def case(name):
    return [c for c in CASES if c.name == name][0]


def par_of(c):
    return Par(w(c.tau), c.powered, c.k, c.k_rows, c.transposed, c.max_iter)


@functools.lru_cache(maxsize=None)
def inputs(c):
    """(s, y) [B, L] fp32: scores N(0, 1) x scale (one slate quantised to quarters: exact ties), labels 0..4, the slates of `zero` all 0;
    pads at the end or interleaved from original index 0 on (evenly spread, so some valid row has an original index >= n)"""
    B, L = len(c.counts), c.L
    if c.pad == "clamp":
        s = np.array([[7.0, 24.0, 0.9, 0.3, -0.4, -1.1], [24.0, 0.9, 0.3, -0.4, -1.1, 7.0]], F)
        y = np.array([[PAD, 2, 0, 1, 3, 1], [2, 0, 1, 3, 1, PAD]], F)
        s.setflags(write=False), y.setflags(write=False)
        return s, y
    rng = np.random.default_rng([L, c.seed, len(c.counts)])
    s = rng.standard_normal((B, L))
    y = rng.integers(0, 5, (B, L)).astype(np.float64)
    for b, n in enumerate(c.counts):
        if c.ties == b:
            s[b] = np.round(s[b] * 4) / 4
        if b in c.zero:
            y[b] = 0
        if c.pad == "inter" and 0 < n < L:
            pads = np.unique(np.floor(np.arange(L - n) * (L / float(L - n))).astype(int))
            assert len(pads) == L - n and pads[0] == 0
            y[b, pads] = float(PAD)
        else:
            y[b, n:] = float(PAD)
    s, y = (s.astype(F) * F(c.scale)).astype(F), y.astype(F)
    s.setflags(write=False), y.setflags(write=False)
    return s, y


@functools.lru_cache(maxsize=None)
def _trace(c):
    """the fp64 residual trace and Zmax of a case (tol 0: every step run)"""
    s, y = inputs(c)
    r = _core(s, y, par_of(c), 0.0, np.float64, "numpy", cond=True)
    return r["res"], float(r["zmax"].max()) if len(r["zmax"]) else 0.0


@functools.lru_cache(maxsize=None)
def tol_of(c):
    if c.T is None:
        return 0.0
    res, zmax = _trace(c)
    tol, ok = derive_tol(res, c.T, max(c.counts), zmax)
    assert ok, "%s: an exit after %d steps cannot be guarded (trace %s)" % (c.name, c.T, res.max(0)[:c.T + 1])
    return tol


@functools.lru_cache(maxsize=None)
def reference(c):
    s, y = inputs(c)
    ref = neural_ref(s, y, par_of(c), tol_of(c))
    assert ref["T"] == (c.max_iter if c.T is None else c.T)
    return ref


def transcription(c, wrong=None):
    s, y = inputs(c)
    return neural_f32(s, y, par_of(c), tol_of(c), wrong)


def checks(got, ref):
    b = bars(ref)
    return {k_: (got[k_], ref[k_], b[k_]) for k_ in ("grad", "per", "loss", "idcg")}


def exact_ok(got, ref):
    return bool(got["T"] == ref["T"] and got["cnt"] == ref["cnt"] and not np.asarray(got["grad"])[ref["zero"]].any()
                and not np.asarray(got["per"])[ref["idcg"] == 0].any())


def measure(cases=None):
    """{output: worst |fp32 - fp64| / (u cond)} of the reference formulation in fp32 over the table and the three orders"""
    out = dict(grad=0.0, per=0.0, loss=0.0, idcg=0.0)
    rows = []
    for c in (cases or CASES):
        s, y = inputs(c)
        ref = reference(c)
        for order in ORDERS:
            got = _core(s, y, par_of(c), tol_of(c), np.float32, order)
            assert got["T"] == ref["T"], (c.name, order, got["T"], ref["T"])
            for k_ in out:
                fl = dict(grad=ref["floor_grad"], per=ref["floor_per"], loss=ref["floor_per"].sum(), idcg=0.0)[k_]
                err = np.maximum(np.abs(f64(got[k_]) - f64(ref[k_])) - fl, 0.0)
                r = worst(err, 0.0 * err, U * f64(ref["cond_" + k_]))
                rows.append((c.name, order, k_, r))
                out[k_] = max(out[k_], r)
    return out, rows


# ---------------------------------------------------------------------------------------------------------------------------------
# ltrx_neuralsort_perturb / ltrx_neuralsort_fold_grad (allrank_amd/csrc/ltrx_neuralsort_stoch.hip) in fp64, with derived bars
# ---------------------------------------------------------------------------------------------------------------------------------
NSORT_PAD = -1.0e30
LOG_EPS = w(1e-10)
P_LOG = 2.0                      # logf: 1 ulp <= 2 u (P_LIBM of tests/step_ref.py)


def perturb_ref(s, y, idcg, cnt, gumbel, beta, log_scores, transposed):
    """s, y [B, L] fp32, gumbel [S, B, L] fp32 -> the outputs of ltrx_neuralsort_perturb; s_pert in fp64 with its bar:
    fl(s + |m|): u |s + |m||; + eps: u; logf: the argument's relative error 2 u through the log is an absolute 2 u (/(1 - 2u)), and P_LOG u
    |log|; fl(beta g): u |beta g|; the last addition: u |s_pert|"""
    s, y, g = np.asarray(s, F), np.asarray(y, F), np.asarray(gumbel, F)
    Sn, B, L = g.shape
    m = F(s.min())
    am = abs(float(m))
    sp = f64(s) + am
    err = U * np.abs(sp)
    if log_scores:
        with np.errstate(divide="ignore", invalid="ignore"):
            lg = np.log(sp + LOG_EPS)
            err = (err + U * (sp + LOG_EPS)) / (sp + LOG_EPS) / (1 - 2 * U) + P_LOG * U * np.abs(lg)
        sp = lg
    bg = w(beta) * f64(g)
    out = sp[None] + bg
    bar = err[None] + U * np.abs(bg) + U * (np.abs(out) + err[None] + U * np.abs(bg))
    i = np.arange(Sn * B)
    bsrc, sort_src = i % B, i // Sn
    yt, ys = y[bsrc], y[sort_src]
    if transposed:
        y_ps = np.where(ys == PAD, F(NSORT_PAD), yt)
    else:
        y_ps = np.where(ys == PAD, PAD, np.where(yt == PAD, F(0), yt))
    return dict(s_pert=out.reshape(Sn * B, L), bar_s_pert=bar.reshape(Sn * B, L), y_ps=y_ps.astype(F), k_rows=(yt != PAD).sum(1).astype(np.int32),
                idcg_ps=np.asarray(idcg, F)[bsrc], cnt_ps=F(F(cnt) * F(Sn)), smin=np.array([m, (s == m).sum()], F))


def gumbel_bar(u):
    """the bar of -logf(-logf(U + 1e-10) + 1e-10) against gumbel_f64(U): the inner log P_LOG u |log| + u (its argument's rounding, absolute
    through the log), the addition u, the outer log that relative error as an absolute one and P_LOG u |log|"""
    x = f64(u) + 1e-10
    inner = -np.log(x)
    e_in = (P_LOG * U * np.abs(inner) + U / (1 - U)) + U * (inner + 1e-10)
    arg = inner + 1e-10
    return e_in / arg / (1 - e_in / arg) + P_LOG * U * np.abs(np.log(arg))


def fold_ref(grad_ps, s, log_scores, k_sum=None):
    """grad_ps [S, B * L], s [B * L] fp32 -> (gradient fp64, bar): S additions (gam(S) on sum |terms|), the weight 1 / ((s + |m|) + eps)
    (4 roundings), the product; sum(gs): k_sum roundings on the longest path of the two-stage sum (a thread's own additions, two block
    sums; n when not given) on sum |gs|, the division by the ties, the last addition"""
    g, s = f64(grad_ps), np.asarray(s, F).ravel()
    Sn, n = g.shape
    m = float(s.min())
    a, aabs = g.sum(0), np.abs(g).sum(0)
    wt = 1.0 / ((f64(s) + abs(m)) + LOG_EPS) if log_scores else np.ones(n)
    gs = a * wt
    e = (Sn + 5) * U * aabs * wt
    tot, etot = gs.sum(), e.sum() + ((n if k_sum is None else k_sum) + 2) * U * (np.abs(gs).sum() + e.sum())
    ties = s == F(m)
    out, bar = gs.copy(), e.copy()
    if m != 0.0:
        add = np.sign(m) * tot / ties.sum()
        out[ties] += add
        bar[ties] += (etot / ties.sum()) * (1 + 2 * U) + 2 * U * abs(add) + U * np.abs(out[ties])
    return out, bar + FLT_MIN
