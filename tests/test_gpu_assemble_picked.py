"""-m gpu: ``ltrx_assemble_batch_picked`` (one launch: host-chosen picks or the stored order -> xb, yb, indices) against its torch
restatement ``DeviceSlates.batch_picked_torch``, bit for bit, on synthetic resident sets:

  * F 136 and 12 (one thread per 16-byte piece of a row), F 9 (scalar form), F 12 with ``x_items`` a view offset by one float (scalar
    form on alignment); L 12 and 64; B 1 and 7;
  * slate lengths 1, L-1, L, L+1, 3L, the batch in non-monotonic slate-id order; picked rows and stored-order rows mixed, among them
    slates of >= L items with ``pick_row`` -1 (their first L items); every picked row holds its slate's LAST position; the rows of the
    pick table in another order than the batch rows;
  * no pick table at all (``picks`` NULL, ``n_pick_rows`` 0); a block of a batch, as a rank passes it;
  * picks taken from ``positions()`` == today's two-launch ``batch()`` for the same seed; the padding branch == ``ltrx_assemble_batch``.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _slates(L, F, seed=0, misalign=False):
    from allrank_amd.data import DeviceSlates
    lens = np.array([L + 1, 1, 3 * L, L - 1, L, 3 * L, L + 1, 2, L])
    rng = np.random.default_rng(seed)
    n = int(lens.sum())
    X = rng.standard_normal((n, F)).astype(np.float32)
    y = rng.integers(0, 5, n).astype(np.float32)
    s = DeviceSlates(X, y, np.repeat(np.arange(len(lens)), lens), device=DEV)
    if misalign:                                            # the same values 4 bytes off a 16-byte boundary
        big = torch.empty(n * F + 1, dtype=torch.float32, device=DEV)
        big[1:] = s.x_items.flatten()
        s.x_items = big[1:].view(n, F)
        assert s.x_items.data_ptr() % 16 == 4 and s.x_items.is_contiguous()
    return s, lens


def _picks(lens, ids, L, rng, stored=()):
    """(pick_row i32[B], picks i32[n, L]): every slate of >= L items is picked (its last position included) unless its batch row is in
    ``stored``; the table's rows are in reverse batch order"""
    rows = [b for b, s in enumerate(ids) if lens[s] >= L and b not in stored]
    table = {}
    for b in rows:
        n = int(lens[ids[b]])
        p = rng.permutation(n)[:L]
        if n - 1 not in p:
            p[int(rng.integers(0, L))] = n - 1
        table[b] = p
    pick_row = np.full(len(ids), -1, dtype=np.int32)
    for r, b in enumerate(reversed(rows)):
        pick_row[b] = r
    picks = np.stack([table[b] for b in reversed(rows)]).astype(np.int32) if rows else np.zeros((0, L), dtype=np.int32)
    return torch.from_numpy(pick_row).to(DEV), torch.from_numpy(picks).to(DEV)


def _equal(a, b):
    assert len(a) == len(b) == 3
    for u, v in zip(a, b):
        assert u.dtype == v.dtype and u.shape == v.shape and torch.equal(u, v)


@pytest.mark.parametrize("B", [1, 7])
@pytest.mark.parametrize("L", [12, 64])
@pytest.mark.parametrize("F,misalign", [(136, False), (12, False), (9, False), (12, True)])
def test_picked_assembly_equals_the_torch_restatement(F, misalign, L, B):
    s, lens = _slates(L, F, misalign=misalign)
    ids = [2, 0, 4, 1, 3, 6, 5][:B]                          # B = 1: the slate of 3L items
    slates = torch.tensor(ids, device=DEV)
    rng = np.random.default_rng(L + B)
    pick_row, picks = _picks(lens, ids, L, rng, stored=(5,))             # row 5 (slate 6, L+1 items) keeps its first L items
    got = s.batch_picked(slates, L, pick_row, picks)
    _equal(got, s.batch_picked_torch(slates, L, pick_row, picks))
    assert got[0].shape == (B, L, F) and got[2].dtype == torch.int64
    last = torch.tensor([int(lens[i]) - 1 for i in ids], device=DEV)
    assert bool(((got[2] == last[:, None]).any(1) | (pick_row < 0)).all())          # the last position of every picked slate
    if B == 7:
        assert torch.equal(got[2][5], torch.arange(L, device=DEV))                   # len >= L, pick_row -1: the first L items
        assert torch.equal(got[0][5], s.x_items[s.offsets[6]:s.offsets[6] + L])
        assert bool((got[1][3][1:] == -1).all()) and bool((got[0][3][1:] == 0).all()) and bool((got[2][3][1:] == -1).all())   # len 1
        # a block of the batch, as a rank passes it: its slates, its pick_row entries, the whole table
        _equal(s.batch_picked(slates[2:5], L, pick_row[2:5], picks), tuple(t[2:5] for t in got))
    # no pick table at all
    none = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    _equal(s.batch_picked(slates, L, none, None), s.batch_picked_torch(slates, L, none, None))


def test_picks_from_the_device_sampler_equal_the_two_launch_batch():
    L, F, seed = 12, 136, 1234
    s, lens = _slates(L, F)
    ids = [2, 0, 4, 1, 3, 6, 5, 8, 7]
    slates = torch.tensor(ids, device=DEV)
    pos = s.positions(slates, L, seed)
    long_rows = [b for b, i in enumerate(ids) if lens[i] >= L]
    pick_row = torch.full((len(ids),), -1, dtype=torch.int32, device=DEV)
    pick_row[long_rows] = torch.arange(len(long_rows), dtype=torch.int32, device=DEV)
    picks = pos[long_rows].to(torch.int32)
    _equal(s.batch_picked(slates, L, pick_row, picks), s.batch(slates, L, seed=seed))
    # the padding branch alone == ltrx_assemble_batch on the positions of the padding branch
    short = torch.tensor([i for i in ids if lens[i] < L], device=DEV)
    none = torch.full((len(short),), -1, dtype=torch.int32, device=DEV)
    _equal(s.batch_picked(short, L, none, None), s.batch(short, L, seed=0))


def test_argument_validation():
    from allrank_amd import _lib as LB
    s, _ = _slates(12, 12)
    lib, one = LB.lib(), torch.zeros(64, dtype=torch.int64, device=DEV)
    p = LB.ptr(one)
    st = LB.stream_of(one)
    assert lib.ltrx_assemble_batch_picked(None, p, p, p, p, None, 0, 1, 12, 12, p, p, p, st) == -1
    assert lib.ltrx_assemble_batch_picked(p, p, p, p, None, None, 0, 1, 12, 12, p, p, p, st) == -1
    assert lib.ltrx_assemble_batch_picked(p, p, p, p, p, None, 1, 1, 12, 12, p, p, p, st) == -1      # NULL picks need n_pick_rows == 0
    assert lib.ltrx_assemble_batch_picked(p, p, p, p, p, None, 0, 0, 12, 12, p, p, p, st) == -1
    assert lib.ltrx_assemble_batch_picked(p, p, p, p, p, None, 0, 1, 0, 12, p, p, p, st) == -1
    with pytest.raises(RuntimeError, match="MI355X only"):
        type(s)(np.zeros((3, 4), np.float32), np.zeros(3, np.float32), np.zeros(3), device="cpu").batch_picked(
            torch.zeros(1, dtype=torch.int64), 2, torch.full((1,), -1, dtype=torch.int32))
