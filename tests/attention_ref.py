"""fp64 reference, entrywise bars, defect models and the case table of the attention contract  --  numpy only, no GPU.

tests/test_attention_ref_cpu.py proves the bars on the CPU (honest fp32 far below them, every defect model above them);
tests/test_gpu_attention_contract.py holds every kernel arm of ltrx_mha.hip / ltrx_mha_res.hip to them.

Reference.  `reference` runs oracle/model_oracle.attention_fwd / attention_bwd in fp64 on q, k, v, dO [.., L, d_k], a key mask and the
keep multipliers of oracle/dropout_oracle.attention_keep_scale, and adds what the bars need: s (scaled, masked scores), m (row
maximum), lse, p, pd = p keep, dP = (dO v^T) keep, delta = sum_j p dP, dS = scale p (dP - delta).  A slate whose keys are all padded
returns zeros for the five tensors and lse 0: what the kernels document (ltrx_mha.hip: "a row whose keys are all padded: 0").

Bars.  First-order rounding bounds, no measured constant.  u(n) = (n + 4) 2^-24 + c_mode is the relative error of an n-term fp32 dot
product against sum |a b| (n additions, the product, three roundings of scaling / storing), plus the per-product error of the
operand split: c_mode = 0 for the exact fp32 MFMA, 3 2^-16 (1 + 2^-7) for three bf16 products, 2 2^-8 (1 + 2^-8) for one (mode 2:
one bf16 rounding, 2^-8, per operand, two operands per product).  Both are the BOUNDS include/ltrx.h states and
tests/test_split_bf16_cpu.py proves: bf16 keeps 8 significand bits, so x = hi + lo leaves up to 2^-16 |x| and the dropped lo lo'
term is up to 2^-16 |x y|.  The 3 2^-18 of ltrx_mha_res.hip's header and the 2^-9 of ltrx.h are the TYPICAL sizes of the same
quantities; a contraction over many keys averages towards them, one over the one or two keys of a short slate does not (the value
row of a length-1 slate comes back as hi + lo exactly, O of a two-key slate carries the roundings of p and v of one product), and
only the bounds hold for every entry.
With Lv the number of valid keys of the slate:

  sigma_ij = u(d_k) scale sum_c |q_ic k_jc|                 the error of one score
  rho_i    = 2 max_j sigma_ij                               p_ij = exp(s_ij - lse_i): a score error moves s_ij and lse_i
             + 2^-23 (max_j |s_ij| + |m_i|)                 s and m each rounded once more in the log2 domain (s log2e, (m + log2 l) ln2)
             + 2^-21                                        the hardware exp2 / log2 (1 ulp each, argument and result rounded)
             + (Lv + 4) 2^-24                               the row sum l of Lv terms
           = the relative error of every p_ij of row i, and the absolute error of lse_i (d lse = sum_j p_ij d s_ij <= max_j):
  bar_lse  = rho
  bar_O    = (pd |v|) (rho + u(Lv))                         O = pd v: the error of pd, and the Lv-term contraction
  bar_dV   = (pd (rho + u(Lv)))^T |dO|                      dV = pd^T dO, likewise
  pi_ij    = u(d_k) (|dO| |v|^T)_ij keep_ij                 the error of dP_ij, a d_k-term contraction
  Delta_i  = sum_j p_ij (pi_ij + rho_i |dP_ij|) + u(Lv) sum_j p_ij |dP_ij|
                                                            delta_i = sum_j p dP, computed as rowsum(dO O) or from p and dP: the errors of
                                                            its factors, and an Lv-term sum
  eps_ij   = scale p_ij (rho_i |dP_ij - delta_i| + pi_ij + Delta_i + 2^-23 (|dP_ij| + |delta_i|))
                                                            dS = scale p (dP - delta): the error of p, of dP, of delta, the subtraction
                                                            and the two multiplications
  bar_dQ   = (eps + u(Lv) |dS|) |k|                         dQ = dS k
  bar_dK   = (eps + u(Lv) |dS|)^T |q|                       dK = dS^T q

Underflow.  The figures above are relative, and fp32 stops being relative below eta = 2^-126: a probability, a dS or an output
entry smaller than that is flushed or loses bits (plain fp32 attention on the CPU already does: with dropout, a row whose dominant
key is dropped keeps only probabilities of 1e-45).  Every p_ij of a valid key therefore carries eta on top of rho_i p_ij, every
dS_ij eta on top of eps_ij, and every output entry of a valid row eta on top of its bar; rows of padded keys and fully padded
slates keep a bar of exactly 0.  At 1e-38 the term decides nothing above the underflow range.

Every other term is a product of a relative rounding figure with the magnitude it acts on, so the bars follow the scale of each entry:
an error confined to a few small entries does not hide behind the largest one.  Mode 2 is outside the parity contract (ltrx.h); it
is held to the same bars with its own c_mode and must FAIL the mode-1 bar on O, which shows that the cases tell one product from three.

Defect models.  `DEFECTS` are reference variants, each a kernel that is subtly wrong in a way these kernels can be wrong.
"""
import math
import os
import re
from collections import namedtuple

import numpy as np

from oracle import dropout_oracle as D
from oracle import model_oracle as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
C_MODE = {0: 0.0, 1: 3.0 * 2.0 ** -16 * (1 + 2.0 ** -7), 2: 2.0 * 2.0 ** -8 * (1 + 2.0 ** -8)}
ETA = 2.0 ** -126                  # the smallest normal fp32 number
LAZY_TAU = 8.0                     # kLazyTau of ltrx_mha_res.hip (log2 units)
TENSORS = ("o", "lse", "dq", "dk", "dv")
SEED = 77


def header_constants():
    """LTRX_MAX_SLATE_LEN and LTRX_MHA_DS_BUDGET_BYTES as include/ltrx.h states them"""
    text = open(os.path.join(ROOT, "include", "ltrx.h")).read()
    out = {}
    for name in ("LTRX_MAX_SLATE_LEN", "LTRX_MHA_DS_BUDGET_BYTES"):
        out[name] = int(re.search(r"#define\s+%s\s+\(?(\d+)" % name, text).group(1))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the dispatch of ltrx_mha_fwd / ltrx_mha_bwd, restated
# ---------------------------------------------------------------------------------------------------------------------
def dkp(dk):
    return (dk + 31) // 32 * 32


def fwd_arm(mode, dk):
    return "res" if mode != 0 and 32 < dk <= 64 else "exact"


def bwd_arm(mode, B, L, h, dk, consts=None):
    c = consts or header_constants()
    lk = (L + 63) // 64 * 64
    fits = fwd_arm(mode, dk) == "res" and L <= c["LTRX_MAX_SLATE_LEN"] and B * h * lk * lk * 4 <= c["LTRX_MHA_DS_BUDGET_BYTES"]
    return "res" if fits else "exact"


def bwd_workspace_bytes(mode, B, L, h, dk, consts=None):
    lk = (L + 63) // 64 * 64
    return B * h * lk * lk * 4 if bwd_arm(mode, B, L, h, dk, consts) == "res" else B * L * h * 4


def arm_name(mode, B, L, h, dk, consts=None):
    f, b = fwd_arm(mode, dk), bwd_arm(mode, B, L, h, dk, consts)
    return f if f == b else "mixed"


def instantiations(mode, B, L, h, dk, p_drop, consts=None):
    """the kernel instantiations one forward + backward call pair launches"""
    drop = int(p_drop > 0)
    pl = int(mode == 2)
    out = set()
    if fwd_arm(mode, dk) == "res":
        out.add("ltrx_mha_fwd_res_kernel<DROP=%d, PL=%d>" % (drop, pl))
    else:
        out.add("ltrx_mha_fwd_kernel<%d, DROP=%d>" % (dkp(dk), drop))
    if bwd_arm(mode, B, L, h, dk, consts) == "res":
        out.add("ltrx_mha_bwd_dkdv_res_kernel<DROP=%d, PL=%d>" % (drop, pl))
        out.add("ltrx_mha_bwd_dq_res_kernel<PL=%d, NW=%d>" % (pl, 4 if L <= 256 else 8))
    else:
        out.add("ltrx_mha_bwd_dq_kernel<%d, DROP=%d>" % (dkp(dk), drop))
        out.add("ltrx_mha_bwd_dkdv_kernel<%d, DROP=%d>" % (dkp(dk), drop))
    return out


def all_instantiations():
    out = set()
    for d in (0, 1):
        for w in (32, 64, 96, 128):
            for kern in ("fwd", "bwd_dq", "bwd_dkdv"):
                out.add("ltrx_mha_%s_kernel<%d, DROP=%d>" % (kern, w, d))
        for pl in (0, 1):
            out.add("ltrx_mha_fwd_res_kernel<DROP=%d, PL=%d>" % (d, pl))
            out.add("ltrx_mha_bwd_dkdv_res_kernel<DROP=%d, PL=%d>" % (d, pl))
    for pl in (0, 1):
        for nw in (4, 8):
            out.add("ltrx_mha_bwd_dq_res_kernel<PL=%d, NW=%d>" % (pl, nw))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------------------------------------------------
Ref = namedtuple("Ref", "o lse dq dk dv s m p pd dP delta dS scale mask keep full")


def _four(x):
    x = np.asarray(x, np.float64)
    return x[None, None] if x.ndim == 2 else x


def reference(q, k, v, do, mask, keep=None):
    """q, k, v, dO [L, d_k] (or [B, h, L, d_k]); mask [L] (or [B, L]) True = padded key; keep [L, L] (or [B, h, L, L]) or None"""
    single = np.asarray(q).ndim == 2
    q, k, v, do = _four(q), _four(k), _four(v), _four(do)
    mask = np.asarray(mask, bool)
    mask = mask[None] if mask.ndim == 1 else mask
    B, h, L, dk = q.shape
    keep = np.ones((B, h, L, L)) if keep is None else np.asarray(keep, np.float64).reshape(B, h, L, L)
    full = mask.all(-1)
    mk = mask.copy()
    mk[full] = False                                       # computed unmasked, zeroed below
    o, p = M.attention_fwd(q, k, v, mk, keep)
    dq, dkk, dv = M.attention_bwd(q, k, v, p, do, keep)
    scale = 1.0 / math.sqrt(dk)
    s = np.where(mk[:, None, None, :], -np.inf, (q @ np.swapaxes(k, -1, -2)) / math.sqrt(dk))
    m = s.max(-1)
    lse = m + np.log(np.exp(s - m[..., None]).sum(-1))
    pd = p * keep
    dP = (do @ np.swapaxes(v, -1, -2)) * keep
    delta = (p * dP).sum(-1)
    dS = scale * p * (dP - delta[..., None])
    parts = [o, lse, dq, dkk, dv, s, m, p, pd, dP, delta, dS]
    for b in np.flatnonzero(full):
        for a in parts:
            a[b] = 0.0
        s[b] = -np.inf
    r = Ref(*parts, scale=scale, mask=mask, keep=keep, full=full)
    if single:
        r = r._replace(**{t: getattr(r, t)[0, 0] for t in TENSORS})
    return r


def bars(ref, q, k, v, do, mode):
    """the entrywise bars of the module docstring for the batched reference `ref` ([B, h, L, ..] arrays)"""
    q, k, v, do = (np.abs(_four(x)) for x in (q, k, v, do))
    c = C_MODE[mode]
    dk = q.shape[-1]
    valid = ~ref.mask[:, None, None, :]                                       # [B, 1, 1, L]
    Lv = valid.sum(-1).astype(np.float64)                                     # [B, 1, 1]
    u_dk = (dk + 4) * U + c
    u_lv = ((Lv + 4) * U + c)                                                 # [B, 1, 1]
    with np.errstate(invalid="ignore"):
        sigma = np.where(valid, u_dk * ref.scale * (q @ np.swapaxes(k, -1, -2)), 0.0)
        smax = np.where(valid, np.abs(ref.s), 0.0).max(-1)
    rho = 2 * sigma.max(-1) + 2 * U * (smax + np.abs(ref.m)) + 2.0 ** -21 + (Lv + 4) * U      # [B, h, L]
    rho[ref.full] = 0.0
    rl = rho + u_lv                                                           # [B, h, L]
    pi = u_dk * (do @ np.swapaxes(v, -1, -2)) * ref.keep
    adP = np.abs(ref.dP)
    eta = ETA * (valid & ~ref.full[:, None, None, None])                      # [B, 1, 1, L]: underflow of p_ij, valid keys only
    rows = np.swapaxes(eta, -1, -2)                                           # [B, 1, L, 1]: underflow of an output row of a valid key
    live = ETA * ~ref.full[:, None, None, None]
    Delta = (ref.p * (pi + rho[..., None] * adP)).sum(-1) + u_lv * (ref.p * adP).sum(-1) + (eta * adP).sum(-1)
    dev = np.abs(ref.dP - ref.delta[..., None])
    eps = ref.scale * (ref.p * (rho[..., None] * dev + pi + Delta[..., None] + 2 * U * (adP + np.abs(ref.delta)[..., None])) + eta * dev) + eta
    e = eps + u_lv[..., None] * np.abs(ref.dS)
    pe = ref.pd * rl[..., None] + eta * ref.keep
    return dict(lse=rho, o=pe @ v + live, dv=np.swapaxes(pe, -1, -2) @ do + rows, dq=e @ k + live, dk=np.swapaxes(e, -1, -2) @ q + rows)


def worst(got, want, bar):
    """(largest error / bar, its index, error, bar); an error where the bar is 0 counts as infinite, NaN as infinite"""
    got = np.asarray(got, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(got - want)
        ratio = np.where(bar > 0, err / bar, np.where(err == 0, 0.0, np.inf))
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    idx = tuple(int(i) for i in np.unravel_index(int(np.argmax(ratio)), ratio.shape))
    return float(ratio[idx]), idx, float(err[idx]), float(bar[idx])


# ---------------------------------------------------------------------------------------------------------------------
# defect models
# ---------------------------------------------------------------------------------------------------------------------
def bf16(x):
    """round to nearest even to 8 significand bits, as the kernels' fp32 -> bf16 conversion does"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    r = ((u >> np.uint32(16)) & np.uint32(1)) + np.uint32(0x7FFF)
    return ((u + r) & np.uint32(0xFFFF0000)).view(np.float32).astype(np.float64)


def _scores(qs, ks, mask, dk):
    return np.where(mask[:, None, None, :], -np.inf, (qs @ np.swapaxes(ks, -1, -2)) / math.sqrt(dk))


def _softmax_fwd(s, v, keep):
    with np.errstate(invalid="ignore", divide="ignore"):
        m = s.max(-1)
        mm = np.where(np.isfinite(m), m, 0.0)
        lt = np.exp(s - mm[..., None]).sum(-1)
        lse = np.where(lt > 0, mm + np.log(lt), 0.0)
        p = np.where(lt[..., None] > 0, np.exp(s - lse[..., None]), 0.0)
    return (p * keep) @ v, lse


def _lazy_fwd(s, v, keep, omit_tile=None):
    """the resident forward's tile loop with its lazy reference (natural-log units); returns O, lse, moved[rows] = the reference of
    the row moved after its first tile, moves[tile] = rows moved at that tile.  omit_tile: the alpha rescale is left out there."""
    L = s.shape[-1]
    tau = LAZY_TAU * math.log(2.0)
    m = np.full(s.shape[:-1], -np.inf)
    l = np.zeros(s.shape[:-1])
    acc = np.zeros(s.shape[:-1] + (v.shape[-1],))
    moved = np.zeros(s.shape[:-1], bool)
    moves = {}
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range((L + 31) // 32):
            sl = slice(32 * t, min(32 * t + 32, L))
            st = s[..., sl]
            mt = st.max(-1)
            grow = mt > m + tau
            mn = np.where(grow, mt, m)
            mref = np.where(np.isfinite(mn), mn, 0.0)
            alpha = np.where(grow, np.exp(m - mref), 1.0)
            second = grow & np.isfinite(m)
            moves[t] = int(second.sum())
            moved |= second
            if t != omit_tile:
                l = l * alpha
                acc = acc * alpha[..., None]
            pt = np.exp(st - mref[..., None])
            l = l + pt.sum(-1)
            acc = acc + (pt * keep[..., sl]) @ v[..., sl, :]
            m = mn
        mm = np.where(np.isfinite(m), m, 0.0)
        o = np.where(l[..., None] > 0, acc / l[..., None], 0.0)
        lse = np.where(l > 0, mm + np.log(l), 0.0)
    return o, lse, moved, moves


def _backward_from(q, k, v, do, s, keep, o, lse, scale):
    """what the backward kernels compute from the saved O and lse: p = exp(s - lse), delta = rowsum(dO O)"""
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.where(np.isfinite(s), np.exp(s - lse[..., None]), 0.0)
    dP = (do @ np.swapaxes(v, -1, -2)) * keep
    delta = (do * o).sum(-1)
    dS = scale * p * (dP - delta[..., None])
    return dS @ k, np.swapaxes(dS, -1, -2) @ q, np.swapaxes(p * keep, -1, -2) @ do


def variant(q, k, v, do, mask, keep, qs=None, ks=None, keep_bwd=None, lazy=None, dk=None):
    """fp64 attention, forward and backward, the way the kernels organise it (backward from the saved O and lse) with the hooks the
    defect models need: qs / ks = the operands of the score product, keep_bwd = the backward's keep multipliers, lazy = None,
    ("omit",) or ("lse",), dk = the head width of the softmax scale.  Without a hook it equals `reference` (tests/test_attention_ref_cpu.py)."""
    q, k, v, do = _four(q), _four(k), _four(v), _four(do)
    B, h, L, _ = q.shape
    dk = dk or q.shape[-1]
    keep = np.ones((B, h, L, L)) if keep is None else np.asarray(keep, np.float64)
    scale = 1.0 / math.sqrt(dk)
    s = _scores(q if qs is None else _four(qs), k if ks is None else _four(ks), np.asarray(mask, bool), dk)
    if lazy is None:
        o, lse = _softmax_fwd(s, v, keep)
    else:
        _, _, moved, moves = _lazy_fwd(s, v, keep)
        later = [t for t in sorted(moves) if t > 0 and moves[t] > 0]
        assert later, "the running reference never moves after the first tile: the lazy defects do not apply"
        if lazy[0] == "omit":
            o, lse, _, _ = _lazy_fwd(s, v, keep, omit_tile=later[-1])
        else:
            o, lse = _softmax_fwd(s, v, keep)
            lse = lse + np.where(moved, LAZY_TAU * math.log(2.0), 0.0)
    dq, dkk, dv = _backward_from(q, k, v, do, s, keep if keep_bwd is None else np.asarray(keep_bwd, np.float64), o, lse, scale)
    return dict(o=o, lse=lse, dq=dq, dk=dkk, dv=dv)


def _d_q_bf16(c, X):
    return variant(X.q, X.k, X.v, X.do, X.mask, X.keep(c.p), qs=bf16(X.q))


def _d_qk_bf16(c, X):
    return variant(X.q, X.k, X.v, X.do, X.mask, X.keep(c.p), qs=bf16(X.q), ks=bf16(X.k))


def _d_tile_skipped(c, X):
    """the last 32-key tile that holds a valid key of slate 0 is never visited (by any slate)"""
    last = int(np.flatnonzero(~X.mask[0])[-1]) // 32
    mask = X.mask.copy()
    mask[:, 32 * last:32 * last + 32] = True
    return variant(X.q, X.k, X.v, X.do, mask, X.keep(c.p))


def _d_alpha_omitted(c, X):
    return variant(X.q, X.k, X.v, X.do, X.mask, X.keep(c.p), lazy=("omit",))


def _d_lse_off(c, X):
    return variant(X.q, X.k, X.v, X.do, X.mask, X.keep(c.p), lazy=("lse",))


def _d_seed_plus_one(c, X):
    return variant(X.q, X.k, X.v, X.do, X.mask, X.keep(c.p), keep_bwd=X.keep(c.p, SEED + 1))


def _d_padded_not_zeroed(c, X):
    """dK / dV rows of padded keys keep what an unmasked pass leaves there"""
    out = variant(X.q, X.k, X.v, X.do, X.mask, X.keep(c.p))
    free = variant(X.q, X.k, X.v, X.do, np.zeros_like(X.mask), X.keep(c.p))
    rows = np.broadcast_to(X.mask[:, None, :, None], out["dk"].shape)
    for t in ("dk", "dv"):
        out[t] = np.where(rows, free[t], out[t])
    return out


def _d_width_padded(c, X):
    """the head is read DKP wide: columns d_k .. DKP-1 hold whatever follows it in the row (here: noise at the operands' scale)"""
    rng = np.random.default_rng(5)
    w = (64 if 32 < c.dk <= 64 else dkp(c.dk)) - c.dk

    def wide(x):
        g = rng.standard_normal(x.shape[:-1] + (w,)) * np.abs(x).mean(-1, keepdims=True)
        return np.concatenate([x.astype(np.float64), g], -1)

    out = variant(wide(X.q), wide(X.k), wide(X.v), wide(X.do), X.mask, X.keep(c.p), dk=c.dk)
    return {t: (a if t == "lse" else a[..., :c.dk]) for t, a in out.items()}


# name -> (model, applies(case with .p set, inputs))
DEFECTS = {
    "q rounded to bf16 in S": (_d_q_bf16, lambda c, X: True),
    "q and k rounded to bf16 in S": (_d_qk_bf16, lambda c, X: True),
    "one 32-key tile skipped": (_d_tile_skipped, lambda c, X: True),
    "one alpha rescale omitted": (_d_alpha_omitted, lambda c, X: c.family == "climbing"),
    "lse off by kLazyTau ln 2": (_d_lse_off, lambda c, X: c.family == "climbing"),
    "backward with the keep mask of seed + 1": (_d_seed_plus_one, lambda c, X: c.p > 0),
    "padded-key dK / dV not zeroed": (_d_padded_not_zeroed, lambda c, X: bool(X.mask.any())),
    "head width read as padded": (_d_width_padded, lambda c, X: c.dk % 32 != 0),
}


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
_Case = namedtuple("Case", "name dk B L h pdrops modes lens maskkind family layouts strides p")


def Case(name, dk, B, L, h, pdrops, modes, lens=None, maskkind="tail", family="scaled", layouts=("padded", "cu"), strides="own"):
    return _Case(name, dk, B, L, h, tuple(pdrops), tuple(modes), lens, maskkind, family, tuple(layouts), strides, None)


def _case_table():
    out = []
    # exact kernels: mode 0 everywhere, mode 1 where it must dispatch the same way (d_k <= 32, d_k > 64)
    for dk, B, L, h, ps in ((4, 2, 33, 2, (0, .3)), (32, 2, 129, 1, (0, .3)), (64, 2, 161, 2, (0, .3)), (68, 2, 130, 1, (0, .1)),
                            (96, 2, 130, 1, (0, .1)), (100, 2, 70, 1, (0, .3)), (124, 2, 70, 1, (0, .3)), (128, 1, 33, 1, (0, .3))):
        lens = [L, 2 * L // 3 + 1][:B]
        out.append(Case("exact dk%d L%d" % (dk, L), dk, B, L, h, ps, (0,) if dk == 64 else (0, 1), lens))
    # resident kernels, modes 1 and 2: one key tile, two, the first tile on ring slots 4-7 (the prologue scratch), the full ring
    # (dq_res NW = 4); then the ring wrap, grid.y = 2, a second row block with one active wave, dq_res NW = 8
    for dk in (36, 60, 64):
        out.append(Case("resident dk%d ragged256" % dk, dk, 5, 256, 2, (0, .3), (1, 2), [1, 32, 33, 129, 256]))
        out.append(Case("resident dk%d ragged289" % dk, dk, 3, 289, 2, (0, .3), (1, 2), [257, 289, 31]))
    # mask shapes (padded layout): one exact and one resident arm each
    for kind in ("first tile", "middle tile", "tail and interior", "slate"):
        out.append(Case("mask %s exact" % kind, 32, 2, 100, 2, (0, .3), (0,), None, kind, layouts=("padded",)))
        out.append(Case("mask %s resident" % kind, 64, 2, 100, 2, (0, .3), (1,), None, kind, layouts=("padded",)))
    out.append(Case("climbing", 64, 2, 240, 2, (0, .3), (0, 1), [240, 230], family="climbing", layouts=("padded",)))
    # resident forward, exact backward: beyond LTRX_MAX_SLATE_LEN, and the smallest shape over the dS budget
    out.append(Case("mixed L2049", 36, 1, 2049, 1, (0, .3), (1, 2), [2049], layouts=("padded",)))
    out.append(Case("mixed budget", 36, 131073, 2, 1, (.3,), (1, 2), "alternate", layouts=("padded",)))
    return [c._replace(strides="engine" if i % 2 else "own") for i, c in enumerate(out)]


CASES = _case_table()


def cpu_core(c):
    """the case as the CPU test runs it: cases longer than 600 items shrink to their B = 1, h = 1 core"""
    return c._replace(B=1, h=1, lens=c.lens[:1]) if c.L > 600 else c


class Inputs(object):
    """q, k, v, dO [B, h, L, d_k] (float32 values), mask [B, L], lens; keep(p) cached.  Inputs are not normalised: per-row scales
    2^-3 .. 2^3 on q and k, independent ones on v and dO.  dO is 0 at padded rows (the loss masks them), as the step has it."""

    def __init__(self, c):
        rng = np.random.default_rng(1000 + sum(map(ord, c.name)))
        B, h, L, dk = c.B, c.h, c.L, c.dk
        self.c = c
        mask = np.zeros((B, L), bool)
        if c.lens == "alternate":
            lens = [2 - (b % 2) for b in range(B)]
            mask[1::2, 1] = True
        elif c.lens is not None:
            lens = list(c.lens)
            for b, n in enumerate(lens):
                mask[b, n:] = True
        else:
            lens = None
            if c.maskkind == "first tile":
                mask[0, :32] = True
                mask[1, :32] = True
                mask[1, 90:] = True
            elif c.maskkind == "middle tile":
                mask[:, 32:64] = True
            elif c.maskkind == "tail and interior":
                mask[0, 77:] = True
                mask[1, 95:] = True
                mask[1, 40] = True
            elif c.maskkind == "slate":
                mask[1, :] = True
                mask[0, 70:] = True
        self.mask, self.lens = mask, lens

        def rows(scaled=True):
            x = rng.standard_normal((B, h, L, dk))
            return (x * 2.0 ** rng.integers(-3, 4, (B, h, L, 1))).astype(np.float32) if scaled else x.astype(np.float32)

        if c.family == "climbing":
            # logits rising by 11 natural units per 32-key tile: test_attention_lazy_softmax_reference_is_invariant_to_the_key_order's
            # construction, with a ramp feature that is no bf16 number (1.7 instead of 2)
            q, k = 0.05 * rows(False), 0.05 * rows(False)
            ramp = (np.arange(L) // 32).astype(np.float32) * np.float32(11.0)
            q[:, :, :, 0] = 1.7
            k[:, :, :, 0] = ramp * np.float32(math.sqrt(dk) / 1.7)
            q[1, :, 100:140, 0] = -1.7                           # these queries see the ramp falling
            self.q, self.k, self.v, self.do = q, k, rows(False), rows(False)
        else:
            self.q, self.k, self.v, self.do = rows(), rows(), rows(), rows()
        self.do = self.do * ~mask[:, None, :, None]
        self._keep = {}

    def keep(self, p, seed=SEED, word=3):
        key = (p, seed)
        if key not in self._keep:
            c = self.c
            self._keep[key] = D.attention_keep_scale(p, seed, word, c.B, c.h, c.L) if p > 0 else None
        return self._keep[key]

    def reference(self, p):
        return reference(self.q, self.k, self.v, self.do, self.mask, self.keep(p))
