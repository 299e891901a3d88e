"""Shared by tests/test_click_cpu.py, tests/test_gpu_click.py and tests/golden/make_golden_clicks.py: the click cases, their inputs, and
a numpy restatement of the four click models (cascade, only-relevant, max-clicks, diverse) with a SEQUENTIAL fp64 distance and numpy's
linear quantile rule written out.  Nothing here imports the reference or allrank_amd.clicks.

A click model is a nested tuple: ("cascade", eta, threshold) | ("relevant", threshold) | ("max", max_clicks, inner) |
("diverse", q, inner).  ``ours`` / ``theirs`` build the allrank_amd.clicks specs / the reference's objects from it.

Data: "lattice" -- features from {-2 .. 2} as float32, so many exact duplicates and exactly tied distances (squared distances are
integers: ties stay ties under any deterministic square root) -- and "gauss", standard normal float32, for which the generator
asserts the gap condition of ``gap_violations``.  Inputs come from the legacy ``np.random.RandomState`` (a frozen stream).
"""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "click_golden.npz")
GAP = 1e-9


def header_constant(name):
    with open(os.path.join(ROOT, "include", "ltrx.h")) as fh:
        return int(re.search(r"#define %s (\d+)" % name, fh.read()).group(1))


LDS_LEN = header_constant("LTRX_CLICK_LDS_SLATE_LEN")          # the longest slate whose distances stay in LDS
LENS = [0, 1, 2, 3, 4, 5, 13, 63, 64, 65]                       # pair counts 0, 0, 1, odd, even, even, ...
SHIPPED = ("diverse", 0.5, ("cascade", 1, 2))                   # scripts/local_config_click_model.json


def _cases():
    out = {}

    def add(name, kind, F, lens, model, seed):
        out[name] = dict(kind=kind, F=F, lens=list(lens), model=model, seed=seed)

    for kind in ("lattice", "gauss"):
        for F in (1, 3, 20, 136):
            if kind == "gauss" and F >= 20:                     # (incompressible: the fixture stays small)
                continue
            add("shipped.%s.F%d" % (kind, F), kind, F, LENS, SHIPPED, 11 + F)
        for q in (0.0, 0.25, 0.5, 0.9, 1.0):
            add("q%g.%s" % (q, kind), kind, 3, LENS, ("diverse", q, ("relevant", 1)), 40 + int(q * 100))
        for thr in (2, 0, -1):
            add("eta05.thr%d.%s" % (thr, kind), kind, 3, LENS, ("diverse", 0.5, ("cascade", 0.5, thr)), 70 + thr)
        add("max_inside.%s" % kind, kind, 3, LENS, ("diverse", 0.25, ("max", 3, ("relevant", 1))), 81)
        add("max_outside.%s" % kind, kind, 3, LENS, ("max", 2, ("diverse", 0.25, ("relevant", 0))), 82)
        add("max_both.%s" % kind, kind, 3, LENS, ("max", 2, ("diverse", 0.25, ("max", 6, ("cascade", 0.5, 1)))), 83)
        add("long.%s" % kind, kind, 8, [300], ("diverse", 0.5, ("relevant", 0)), 90)
        add("lds_edge.%s" % kind, kind, 4, [LDS_LEN, LDS_LEN + 1], ("diverse", 0.5, ("relevant", 1)), 91)
    add("plain.cascade", "lattice", 3, LENS, ("cascade", 1, 2), 84)
    add("plain.max.cascade", "lattice", 3, LENS, ("max", 3, ("cascade", 0.5, 0)), 85)
    add("plain.relevant", "lattice", 3, LENS, ("relevant", 2), 86)
    short = np.random.RandomState(7).randint(0, 7, 300)
    add("many_short", "lattice", 5, short, ("diverse", 0.5, ("cascade", 0.5, 1)), 92)
    return out


CASES = _cases()


def inputs(case):
    """X [N, L, F] float32 (0 on padding), y [N, L] float32 (-1 on padding) of a case"""
    c = CASES[case]
    rs = np.random.RandomState(1000 + c["seed"])
    lens, F = c["lens"], c["F"]
    L = max(max(lens), 1)
    if c["kind"] == "lattice":
        X = rs.randint(-2, 3, (len(lens), L, F)).astype(np.float32)
    else:
        X = rs.standard_normal((len(lens), L, F)).astype(np.float32)
    y = rs.randint(0, 5, (len(lens), L)).astype(np.float32)
    for b, n in enumerate(lens):
        X[b, n:], y[b, n:] = 0, -1
    return X, y


def uniforms(case):
    """the uniforms a cascade consumes under np.random.seed(seed): one per valid item, in slate order (empty for only-relevant)"""
    c = CASES[case]
    return np.random.RandomState(c["seed"]).rand(sum(c["lens"])) if draws(c["model"]) else np.zeros(0)


def draws(model):
    return model[0] == "cascade" or (model[0] in ("max", "diverse") and draws(model[2]))


def is_diverse(model):
    return model[0] == "diverse" or (model[0] == "max" and is_diverse(model[2]))


def ours(model):
    from allrank_amd import clicks as C
    if model[0] == "cascade":
        return C.Cascade(model[1], model[2])
    if model[0] == "relevant":
        return C.OnlyRelevant(model[1])
    if model[0] == "max":
        return C.MaxClicks(ours(model[2]), model[1])
    return C.Diverse(ours(model[2]), model[1])


def theirs(model):
    """the reference's objects (the reference must be loaded)"""
    from allrank.click_models.base import MaxClicksModel, OnlyRelevantClickModel
    from allrank.click_models.cascade_models import BaseCascadeModel, DiverseClicksModel
    if model[0] == "cascade":
        return BaseCascadeModel(model[1], model[2])
    if model[0] == "relevant":
        return OnlyRelevantClickModel(model[1])
    if model[0] == "max":
        return MaxClicksModel(theirs(model[2]), model[1])
    return DiverseClicksModel(theirs(model[2]), model[1])


# ------------------------------------------------------------------------------------------------------------------
# the restatement
# ------------------------------------------------------------------------------------------------------------------
def distances(X):
    """[n, n] fp64 Euclidean distances, the squares of the differences added over k ascending, one rounding per operation"""
    X = np.asarray(X, dtype=np.float64)
    s = np.zeros((X.shape[0], X.shape[0]), dtype=np.float64)
    for k in range(X.shape[1]):
        d = X[:, None, k] - X[None, :, k]
        s = s + d * d
    return np.sqrt(s)


def margin_of(dist, q):
    """numpy's linear quantile of the pairs i < j, written out; 0 without a pair"""
    n = dist.shape[0]
    if n < 2:
        return 0.0
    s = np.sort(dist[np.triu_indices(n, 1)])
    N = s.shape[0]
    v = np.float64(q) * np.float64(N - 1)
    lo = int(np.floor(v))
    hi = min(lo + 1, N - 1)
    t = v - np.float64(lo)
    a, b = s[lo], s[hi]
    return float(a + (b - a) * t) if t < 0.5 else float(b - (b - a) * (np.float64(1.0) - t))


def restate(model, X, y, rand=None, used=None):
    """bool clicks of one slate's valid items X [n, F], y [n]; a cascade draws from ``rand`` (default: the global numpy generator).
    ``used``: a list that receives (distance, margin, is the margin's own pair) of every greedy comparison"""
    rand = np.random.rand if rand is None else rand
    n = len(y)
    if model[0] == "cascade":
        observed = (1 / np.arange(1, n + 1) ** model[1]) >= rand(n)
        return np.where(observed, y, np.float32(0)) >= np.float32(model[2])
    if model[0] == "relevant":
        return y >= np.float32(model[1])
    if model[0] == "max":
        c = restate(model[2], X, y, rand, used)
        return c & (np.cumsum(c) <= model[1])
    dist = distances(X)
    margin = margin_of(dist, model[1])
    c = restate(model[2], X, y, rand, used).copy()
    kept = []
    for i in np.flatnonzero(c):
        ok = True
        for j in kept:                                         # (every clicked item, no early exit: `used` sees them all)
            if used is not None:
                used.append((dist[j, i], margin))
            ok = ok and dist[j, i] > margin
        if ok:
            kept.append(i)
        else:
            c[i] = False
    return c


def margin_model(model):
    return model if model[0] == "diverse" else (margin_model(model[2]) if model[0] == "max" else None)


def restate_batch(model, X, y, rand=None, used=None):
    """(clicks [N, L] float32 with -1 on padding, margins [N] fp64) of a padded batch, slates in order"""
    N, L = y.shape
    clicks = np.full((N, L), -1.0, dtype=np.float32)
    margins = np.zeros(N, dtype=np.float64)
    dm = margin_model(model)
    for b in range(N):
        valid = y[b] != -1
        clicks[b, valid] = restate(model, X[b][valid], y[b][valid], rand, used)
        if dm is not None:
            margins[b] = margin_of(distances(X[b][valid]), dm[1])
    return clicks, margins


def gap_violations(used):
    """the greedy comparisons whose distance is within GAP x margin of the margin without being EQUAL to it (an equal distance is
    the margin's own pair for an odd pair count, or an exact tie)"""
    return [(d, m) for d, m in used if d != m and abs(d - m) <= GAP * m]


def golden():
    return dict(np.load(GOLDEN, allow_pickle=False))


def state_digest(state=None):
    """sha256 of the global numpy generator's state (or of ``state``): what the fixture stores of it, 64 characters instead of 2.5 KB"""
    import hashlib
    kind, keys, pos = (np.random.get_state() if state is None else state)[:3]
    return hashlib.sha256(kind.encode() + np.asarray(keys, dtype=np.uint32).tobytes() + b"%d" % int(pos)).hexdigest()
