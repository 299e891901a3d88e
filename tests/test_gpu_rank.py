"""-m gpu: ltrx_rank_slates_cu against numpy, and the surface around it (allrank_amd.inference: rank_slates on the packed scorer, the
module-path fallbacks, the golden ranking of the reference)."""
import copy
import functools
import types

import numpy as np
import pytest
import torch

from tests import rank_cases as RC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# wave (64) and workgroup (256 / 1024 threads) edges, and more than one item per thread in the counting pass
LENS = [0, 1, 2, 63, 64, 65, 256, 257, 1025]
MAX_LEN = max(LENS)
CANARY = 0xDEADBEEF


def _canary(*shape):
    return torch.from_numpy(np.full(shape, CANARY, dtype=np.uint32).view(np.float32)).to(DEV)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _scores(kind, seed):
    """packed scores of LENS: "ties" -- normal draws quantised to 8 levels, with +0.0 / -0.0 and +-inf planted; "distinct" -- a
    shuffle of distinct values"""
    rng = np.random.default_rng(seed)
    out = []
    for n in LENS:
        if kind == "distinct":
            s = (rng.permutation(n).astype(np.float32) - n / 2) * 0.25
        else:
            s = np.floor(np.clip(rng.standard_normal(n), -2, 1.999) * 2).astype(np.float32) / 2 + 0.25   # -1.75 .. 1.75: 8 levels
            if n >= 63:
                pos = rng.permutation(n)[:8]
                s[pos[:2]], s[pos[2:4]] = 0.0, -0.0
                s[pos[4:6]], s[pos[6:8]] = np.inf, -np.inf
        out.append(s.astype(np.float32))
    return out


@functools.lru_cache(maxsize=None)
def _case(F, L, kind):
    """inputs in both source forms and the expected outputs, computed once per case and never modified"""
    B = len(LENS)
    sc = _scores(kind, 11)
    cu = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int32)
    n = int(cu[-1])
    # sentinel features: every (slate, item, column) its own bit pattern (floats > 1, no NaN), so that a wrong row cannot match;
    # the padded slots of the grid hold junk that must not reach the output
    x = (np.arange(B * L * F, dtype=np.uint32) + np.uint32(0x3F800000)).reshape(B, L, F)
    y = (np.arange(B, dtype=np.float32)[:, None] * 2048 + np.arange(L, dtype=np.float32)[None, :])
    for b, k in enumerate(LENS):
        y[b, k:] = -1
    # the resident set: the same items as CSR rows, stored in another slate order than the batch's, and one slate the batch skips
    store = [4, 8, 1, 6, 2, 7, 3, 5]                                        # batch slates with items, in stored order
    offs, ids, rows_x, rows_y = [0], np.zeros(B, dtype=np.int64), [], []
    extra = np.full((5, F), 0x40400000, dtype=np.uint32)                    # a slate of 5 items that no id names
    for pos, b in enumerate(store):
        if pos == 3:
            rows_x.append(extra), rows_y.append(np.full(5, 77, np.float32)), offs.append(offs[-1] + 5)
        ids[b] = len(offs) - 1
        rows_x.append(x[b, :LENS[b]]), rows_y.append(y[b, :LENS[b]]), offs.append(offs[-1] + LENS[b])
    ids[0] = 3                                                              # the empty slate: any id, its cu extent is 0
    exp_x, exp_y, perm = np.zeros((B, L, F), np.uint32), np.full((B, L), -1, np.float32), np.zeros(n, np.int32)
    for b, k in enumerate(LENS):
        o = np.argsort(-sc[b], kind="stable")
        perm[cu[b]:cu[b] + k] = o
        exp_x[b, :k], exp_y[b, :k] = x[b, :k][o], y[b, :k][o]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return types.SimpleNamespace(
        B=B, F=F, L=L, n=n, scores=t(np.concatenate(sc)), cu=t(cu), x=t(x.view(np.float32)), y=t(y),
        slates=types.SimpleNamespace(x_items=t(np.concatenate(rows_x).view(np.float32)), y_items=t(np.concatenate(rows_y)),
                                     offsets=t(np.asarray(offs, dtype=np.int64))),
        ids=t(ids), exp_x=exp_x, exp_y=exp_y, perm=perm)


def _run(c, form, order=None, slots=None, scores=None, slates=None):
    """one launch into canary-filled buffers of ``slots`` slates; (perm, x_out, y_out)"""
    from allrank_amd import _lib as LB, inference as EI
    slots = c.B if slots is None else slots
    x_out, y_out = _canary(slots, c.L, c.F), _canary(slots, c.L)
    perm = torch.full((c.n,), -7, dtype=torch.int32, device=DEV)
    src = dict(x=c.x, y=c.y) if form == "grid" else dict(slates=slates or c.slates, ids=c.ids)
    EI.rank_slates_cu(LB.lib(), LB.stream_of(x_out), c.scores if scores is None else scores, c.cu, order, c.B, MAX_LEN, c.L, x_out, y_out,
                      perm, **src)
    torch.cuda.synchronize()
    return perm, x_out, y_out


def _assert_exact(c, got, slates=None):
    perm, x_out, y_out = got
    sl = slice(None) if slates is None else slates
    assert np.array_equal(_bits(x_out)[:c.B][sl], c.exp_x[sl])
    assert np.array_equal(y_out.cpu().numpy()[:c.B][sl], c.exp_y[sl])


@pytest.mark.parametrize("kind", ["ties", "distinct"])
@pytest.mark.parametrize("L", [MAX_LEN, MAX_LEN + 7])
@pytest.mark.parametrize("F", [1, 3, 136])
def test_kernel_equals_numpy_in_both_source_forms_and_any_launch_order(F, L, kind):
    """perm == np.argsort(-s, kind="stable") per slate; x_out as bit patterns, y_out and both tails exact; grid and resident sources,
    slate_order None and shuffled all give the same bytes.  F = 1 and 3: unaligned rows, 4-byte accesses; F = 136: 16-byte accesses.
    Can a resident F = 136 row start off 16-byte alignment?  Not through its offsets: a row starts (offsets[id] + i) * 544 bytes
    = 34 * 16 behind x_items, whatever the offsets hold (any F % 4 == 0).  Only a misaligned x_items base does it -- the next test."""
    c = _case(F, L, kind)
    grid = _run(c, "grid")
    assert np.array_equal(grid[0].cpu().numpy(), c.perm)
    _assert_exact(c, grid)
    for b, k in enumerate(LENS):                                             # the tails, spelled out
        assert not _bits(grid[1])[b, k:].any() and (grid[2][b, k:] == -1).all()
    order = torch.tensor(np.random.default_rng(5).permutation(c.B).astype(np.int32), device=DEV)
    for other in (_run(c, "grid", order=order), _run(c, "resident"), _run(c, "resident", order=order)):
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(grid, other))


def test_resident_rows_off_16_byte_alignment_take_the_dword_path():
    """x_items one float behind an aligned address (F = 136): every row is 4 bytes off, the call moves dwords -- same bytes out"""
    c = _case(136, MAX_LEN, "ties")
    buf = torch.empty(c.slates.x_items.numel() + 4, dtype=torch.float32, device=DEV)
    off = buf[1:1 + c.slates.x_items.numel()].view(c.slates.x_items.shape)
    off.copy_(c.slates.x_items)
    assert off.data_ptr() % 16 == 4
    sl = types.SimpleNamespace(x_items=off, y_items=c.slates.y_items, offsets=c.slates.offsets)
    got = _run(c, "resident", slates=sl)
    assert np.array_equal(got[0].cpu().numpy(), c.perm)
    _assert_exact(c, got)


@pytest.mark.parametrize("lens,F", [([65, 0, 64, 256], 3), ([6200, 5, 0], 4)])
def test_kernel_at_the_launchers_other_shapes(lens, F):
    """the two launch decisions the main cases do not reach: max_len <= 256 runs 4 waves per slate instead of 16, and max_len = 6200
    takes 2 x 4 x 6200 bytes of dynamic LDS, above the default allowance (the opt-in of ltrx_allow_dynamic_lds)"""
    from allrank_amd import _lib as LB, inference as EI
    rng = np.random.default_rng(len(lens))
    B, L, n = len(lens), max(lens) + 1, sum(lens)
    s = np.floor(rng.standard_normal(n) * 64).astype(np.float32) / 64                  # ties in the long slate
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    x = (np.arange(B * L * F, dtype=np.uint32) + np.uint32(0x3F800000)).reshape(B, L, F)
    y = np.arange(B * L, dtype=np.float32).reshape(B, L)
    exp_x, exp_y, exp_p = np.zeros_like(x), np.full((B, L), -1, np.float32), np.zeros(n, np.int32)
    for b, k in enumerate(lens):
        o = np.argsort(-s[cu[b]:cu[b + 1]], kind="stable")
        exp_p[cu[b]:cu[b + 1]], exp_x[b, :k], exp_y[b, :k] = o, x[b, :k][o], y[b, :k][o]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    x_out, y_out, perm = _canary(B, L, F), _canary(B, L), torch.full((n,), -7, dtype=torch.int32, device=DEV)
    EI.rank_slates_cu(LB.lib(), LB.stream_of(x_out), t(s), t(cu), None, B, max(lens), L, x_out, y_out, perm, x=t(x.view(np.float32)), y=t(y))
    torch.cuda.synchronize()
    assert np.array_equal(perm.cpu().numpy(), exp_p)
    assert np.array_equal(_bits(x_out), exp_x) and np.array_equal(y_out.cpu().numpy(), exp_y)


def test_slots_beyond_the_batch_and_refused_calls_keep_the_canary():
    from allrank_amd import _lib as LB
    c = _case(3, MAX_LEN + 7, "ties")
    perm, x_out, y_out = _run(c, "grid", slots=c.B + 2)
    _assert_exact(c, (perm, x_out, y_out))
    assert (_bits(x_out)[c.B:] == CANARY).all() and (_bits(y_out)[c.B:] == CANARY).all()
    # refused: L < max_len, both source forms, neither, max_len above the limit -- nothing is written
    lib, P = LB.lib(), LB.ptr
    x_out, y_out = _canary(c.B, c.L, c.F), _canary(c.B, c.L)
    perm = torch.full((c.n,), -7, dtype=torch.int32, device=DEV)
    s = c.slates

    def call(x, y, xi, yi, offs, ids, max_len, L):
        return lib.ltrx_rank_slates_cu(P(c.scores), P(x), P(y), P(xi), P(yi), P(offs), P(ids), P(c.cu), None, c.B, max_len, c.F, L, P(perm),
                                       P(x_out), P(y_out), LB.stream_of(x_out))
    assert call(c.x, c.y, None, None, None, None, MAX_LEN, MAX_LEN - 1) == -1
    assert call(c.x, c.y, s.x_items, s.y_items, s.offsets, c.ids, MAX_LEN, c.L) == -1
    assert call(None, None, None, None, None, None, MAX_LEN, c.L) == -1
    assert call(c.x, c.y, None, None, None, None, LB.MAX_METRIC_SLATE_LEN + 1, LB.MAX_METRIC_SLATE_LEN + 1) == -2
    torch.cuda.synchronize()
    assert (_bits(x_out) == CANARY).all() and (_bits(y_out) == CANARY).all() and (perm == -7).all()


@pytest.mark.parametrize("form", ["grid", "resident"])
def test_nan_scores_stay_inside_their_slate_and_every_element_is_written(form):
    """NaNs planted in one slate: its order is unspecified, but its outputs hold no canary and its neighbours are exact"""
    c = _case(136, MAX_LEN + 7, "ties")
    b = LENS.index(65)
    s = c.scores.clone()
    lo = int(c.cu[b])
    s[lo + 3], s[lo + 40], s[lo + 64] = float("nan"), float("nan"), float("nan")
    perm, x_out, y_out = _run(c, form, scores=s, slots=c.B + 1)
    others = [i for i in range(c.B) if i != b]
    _assert_exact(c, (perm, x_out, y_out), others)
    assert not (_bits(x_out)[b] == CANARY).any() and not (_bits(y_out)[b] == CANARY).any()
    assert (_bits(x_out)[c.B:] == CANARY).all()
    p = perm.cpu().numpy()[lo:lo + 65]
    assert ((p >= -1) & (p < 65)).all()


# ------------------------------------------------------------------------------------------------------------------
# the surface
# ------------------------------------------------------------------------------------------------------------------
def _model(F=24, d=32, h=2, N=1, act=None, out_act=None, d_output=1):
    from allrank_amd.model import make_model
    torch.manual_seed(7)
    return make_model(dict(sizes=[d], input_norm=False, activation=act, dropout=0.0),
                      dict(N=N, d_ff=64, h=h, positional_encoding=None, dropout=0.1),
                      dict(d_output=d_output, output_activation=out_act), F).to(DEV)


def _padded(lens, L, F, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((len(lens), L, F)).astype(np.float32)
    y = rng.integers(0, 5, (len(lens), L)).astype(np.float32)
    for b, k in enumerate(lens):
        x[b, k:], y[b, k:] = 0, -1
    return x, y


def _device_slates(x, y, lens):
    from allrank_amd.data import DeviceSlates
    X = np.concatenate([x[b, :k] for b, k in enumerate(lens)])
    Y = np.concatenate([y[b, :k] for b, k in enumerate(lens)])
    return DeviceSlates(X, Y, np.repeat(np.arange(len(lens)), lens), device=DEV)


def _gather_by(scores, x, y):
    """torch.gather by torch.sort(stable=True) of grid scores with padding at -inf"""
    s = scores.clone()
    s[y == -1] = float("-inf")
    _, idx = s.sort(descending=True, dim=-1, stable=True)
    return torch.gather(x, 1, idx.unsqueeze(-1).expand(-1, -1, x.shape[-1])), torch.gather(y, 1, idx)


@pytest.mark.parametrize("L,lens", [(40, [40, 3, 17, 0, 39]), (300, [300, 1, 150, 0, 77])])
def test_rank_slates_equals_gather_by_the_scorers_own_scores(L, lens):
    """both dataset forms == torch.gather by torch.sort(stable=True) of the scorer's own grid scores (a twin engine over a copy of the
    model: the kernels are deterministic), bit for bit in X and y; the fused engine ran"""
    from allrank_amd import inference as EI
    model = _model()
    x, y = _padded(lens, L, 24, L)
    twin = EI.Ranker(copy.deepcopy(model))
    assert twin.reason == ""
    xd, yd = torch.tensor(x, device=DEV), torch.tensor(y, device=DEV)
    sc = twin.scorer(8, L)
    sc.run(xd, yd, None, lengths=torch.tensor(lens, dtype=torch.int32))
    exp_x, exp_y = _gather_by(sc.scores[:len(lens)], xd, yd)
    out = EI.rank_slates({"vali": RC.HostSlates(x, y)}, model, RC.config(8))["vali"]
    assert EI.last_run == {"engine": "fused", "reason": ""}
    assert not out[0].is_cuda and out[0].dtype == torch.float32 and out[1].dtype == torch.float32
    assert np.array_equal(_bits(out[0]), _bits(exp_x)) and np.array_equal(out[1].numpy(), exp_y.cpu().numpy())
    # the resident form: the same slates without the empty one (a stored set has none), in dataset order
    keep = [b for b, k in enumerate(lens) if k]
    ds = _device_slates(x, y, lens)
    assert ds.longest_query_length == L
    res = EI.rank_slates({"vali": ds}, model, RC.config(8))["vali"]
    assert EI.last_run == {"engine": "fused", "reason": ""}
    assert np.array_equal(_bits(res[0]), _bits(exp_x)[keep]) and np.array_equal(res[1].numpy(), exp_y.cpu().numpy()[keep])


@pytest.mark.parametrize("name", ["ordinal", "refused"])
def test_models_the_scorer_cannot_serve_take_the_module_path_with_a_reason(name):
    """d_output = 3, and a model the fused engine refuses (FC activation ELU): the module path's result, never an exception"""
    from allrank_amd import inference as EI
    model = _model(d_output=3, out_act="Sigmoid") if name == "ordinal" else _model(act="ELU")
    lens, L = [40, 3, 17, 39], 40
    x, y = _padded(lens, L, 24, 3)
    xd, yd = torch.tensor(x, device=DEV), torch.tensor(y, device=DEV)
    model.eval()
    with torch.no_grad():
        s = model.score(xd, yd == -1, torch.ones_like(yd).long())
    exp_x, exp_y = _gather_by(s, xd, yd)
    for ds in (RC.HostSlates(x, y), _device_slates(x, y, lens)):
        out = EI.rank_slates({"test": ds}, model, RC.config(8))["test"]
        assert EI.last_run["engine"] == "module" and EI.last_run["reason"]
        assert ("d_output" in EI.last_run["reason"]) == (name == "ordinal")
        assert np.array_equal(_bits(out[0]), _bits(exp_x)) and np.array_equal(out[1].numpy(), exp_y.cpu().numpy())


@pytest.mark.parametrize("form", ["host", "resident"])
def test_engine_ranking_equals_the_reference_golden(form):
    """tests/golden/rank_golden.npz: the reference's own rank_slates on CPU (two batches, a fixed positional encoding fed with ones).
    Adjacent reference scores are >= 1e-3 * max(1, max|s|) apart, 50 x the scorer's bar: the stored order is the engine's, exactly"""
    from allrank_amd import inference as EI
    g = RC.golden()
    model = RC.golden_model(g, DEV)
    lens = [int(k) for k in g["lens"]]
    ds = RC.HostSlates(g["x"], g["y"]) if form == "host" else _device_slates(g["x"], g["y"], lens)
    X, y = EI.rank_slates({"test": ds}, model, RC.config(int(g["cfg.batch_size"])))["test"]
    assert EI.last_run == {"engine": "fused", "reason": ""}
    assert str(X.dtype) == str(g["dtype_x"]) and str(y.dtype) == str(g["dtype_y"])
    assert np.array_equal(_bits(X), g["ranked_x"].view(np.uint32)) and np.array_equal(y.numpy(), g["ranked_y"])
