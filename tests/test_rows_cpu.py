"""allrank_amd/rows.py without a GPU: the device count of the cu_seqlens staging is torch only, so it runs on CPU tensors, and it
must write what the host half of the stager (``_stage_host``) writes for the same slate lengths -- ties in the stable longest-first
order included.  The movers' layout decisions are held with a recording stand-in for the library."""
import ctypes

import numpy as np
import torch

from allrank_amd import engine, rows as RW


def _valid(lens, L, n_slates=None):
    lens = list(lens)[:n_slates]
    return torch.arange(L)[None, :] < torch.tensor(lens, dtype=torch.int64)[:, None]


def _count(valid, B, want=("n", "max_len", "prefix_ok")):
    cu, order = torch.full((B + 1,), -7, dtype=torch.int32), torch.full((B,), -7, dtype=torch.int32)
    got = RW.count_valid(valid, cu, order, want)
    assert list(got) == list(want) and all(v.dim() == 0 and v.dtype == torch.int32 for v in got.values())
    return cu.tolist(), order.tolist(), {k: int(v) for k, v in got.items()}


def test_engine_re_exports_the_moved_names():
    assert engine.row_bucket is RW.row_bucket and engine._stage_host is RW._stage_host and engine._Stager is RW._Stager


def test_count_valid_small_case():
    cu, order, got = _count(_valid([5, 0, 3, 1], 5), 4)
    assert cu == [0, 5, 5, 8, 9] and order == [0, 2, 3, 1]
    assert got == dict(n=9, max_len=5, prefix_ok=1)
    assert _count(_valid([5, 0, 3, 1], 5), 4, want=("n",))[2] == dict(n=9)          # only what the caller asks for


def test_count_valid_sees_interior_padding():
    valid = _valid([5, 0, 3, 1], 5)
    valid[2] = torch.tensor([True, False, True, False, False])          # valid at positions 0 and 2 only
    cu, order, got = _count(valid, 4)
    assert got["prefix_ok"] == 0 and got["n"] == 8 and cu == [0, 5, 5, 7, 8]


def test_count_valid_short_batch_pads_with_empty_slates():
    cu, order, got = _count(_valid([3, 4], 5), 4)
    assert cu == [0, 3, 7, 7, 7] and order == [1, 0, 2, 3] and got == dict(n=7, max_len=4, prefix_ok=1)


def test_count_valid_equals_the_host_stager():
    rng = np.random.default_rng(20)
    for _ in range(200):
        B, L = int(rng.integers(1, 9)), int(rng.integers(1, 13))
        n_sl = int(rng.integers(1, B + 1))
        lens = rng.integers(0, min(L, 3) + 1, n_sl) if rng.random() < 0.7 else rng.integers(0, L + 1, n_sl)     # few values: many ties
        host = torch.full((2 * B + 1,), -7, dtype=torch.int32)
        n = RW._stage_host(host, B, torch.tensor(lens, dtype=torch.int32))
        cu, order, got = _count(_valid(lens, L), B)
        assert cu + order == host.tolist(), (lens, B)
        assert got == dict(n=n, max_len=int(lens.max()), prefix_ok=1)


class _Set(object):
    """the fields of a buffer set the movers read"""

    def __init__(self, layout, saved=True, rows=32, n_valid=11):
        B, L = 3, 5
        self.layout, self.saved, self.B, self.L, self.rows, self.n_valid, self.cap = layout, saved, B, L, rows, n_valid, 64
        self.cu, self.idx = torch.zeros(B + 1, dtype=torch.int32), torch.zeros(64, dtype=torch.int32)
        self.scores_raw, self.dsc_c = torch.ones(B, L), torch.zeros(64)


class _Names(object):
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append(name)
            return 0
        return call


def _moves(bs):
    lib, st = _Names(), ctypes.c_void_p(1)
    o, dqkv, dsc = torch.ones(64, 8), torch.ones(64, 24), torch.ones(bs.B, bs.L)
    RW.zero_attention_tail(bs, lib, st, o)
    RW.scores_to_grid(bs, lib, st, torch.zeros(64), 1)
    back = RW.grid_to_rows(bs, lib, st, dsc, 1)
    RW.zero_gradient_tail(bs, lib, st, dqkv)
    return lib.calls, back is dsc, dqkv


def test_each_layout_moves_its_own_way():
    calls, same, dqkv = _moves(_Set("grid"))
    assert calls == [] and same and float(dqkv.min()) == 1.0
    bs = _Set("index")
    calls, same, dqkv = _moves(bs)
    assert calls == ["ltrx_scatter_rows", "ltrx_gather_rows"] and not same
    assert float(bs.scores_raw.abs().max()) == 0.0                                   # zeroed before the scatter
    assert float(dqkv[:11].min()) == 1.0 and float(dqkv[11:32].abs().max()) == 0.0 and float(dqkv[32:].min()) == 1.0
    calls, same, dqkv = _moves(_Set("cu"))
    assert calls == ["ltrx_zero_rows_cu", "ltrx_scatter_rows_cu", "ltrx_gather_rows_cu", "ltrx_zero_rows_cu"] and not same
    calls, same, dqkv = _moves(_Set("cu", saved=False))                              # the scorer's set: no backward reads ``o``
    assert calls[:2] == ["ltrx_scatter_rows_cu", "ltrx_gather_rows_cu"]


def test_set_rows_is_the_ladder_capped_at_the_allocation():
    bs = _Set("cu")
    for n in (0, 1, 32, 33, 64, 1000):
        RW.set_rows(bs, n)
        assert bs.n_valid == n and bs.rows == RW.row_bucket(max(n, 1), bs.cap)
