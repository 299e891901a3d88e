"""``DeviceLoader(sampling="reference")``: the reference's own FixLength draws (dataset_loading.py:61-79) made on the host, CPU half.

The restated host loader oracle/loader_oracle.py (pinned to the reference's loaders bit for bit by tests/test_loader_cpu.py) is the
reference here: same seeds (main.py:36-38) -> the same ``x``, ``y`` and ``indices`` in every batch, sampled rows included and in
the sampled ORDER (no canonical re-ordering), and the same states of torch's and numpy's global generators afterwards, for
``num_workers`` 0 (draws from numpy's global generator), 1 and 2 (draws from the workers' generators).  The batch assembly itself is
the HIP kernel's job (tests/test_gpu_assemble_picked.py, tests/test_gpu_sampling_loader.py); here its torch restatement
``DeviceSlates.batch_picked_torch`` is injected in its place.
"""
import importlib
import os

import numpy as np
import pytest
import torch

from oracle import loader_oracle as LO
from oracle.ref_loader import reference_available
from tests.test_loader_cpu import _write, _seed, _epochs, _same

L = 12
LONG = {3: 33, 8: 12, 20: 60, 5: 40}
WORKERS = (0, 1, 2)


def write_sampled_job(tmp_path):
    """``_write``'s files with slate 20 (60 items) holding a single label 1 and slate 5 (40 items) two non-zero labels, so that a draw
    without a relevant item meets both relevance branches (:72-74 the only relevant item is kept, :75-76 the draw is repeated)"""
    from sklearn.datasets import dump_svmlight_file, load_svmlight_file
    path = _write(tmp_path, n_q=33, long=LONG)
    for role in ("train", "vali"):
        f = os.path.join(path, "%s.txt" % role)
        X, y, qid = load_svmlight_file(f, query_id=True)
        a = np.flatnonzero(qid == 520)
        y[a] = 0
        y[a[41]] = 1
        b = np.flatnonzero(qid == 505)
        y[b] = 0
        y[b[[7, 29]]] = [2, 1]
        dump_svmlight_file(X, y, f, query_id=qid)
    return path


@pytest.fixture
def torch_assembly(monkeypatch):
    """DeviceSlates.batch_picked -> its torch restatement (no GPU here)"""
    from allrank_amd.data import DeviceSlates
    monkeypatch.setattr(DeviceSlates, "batch_picked", DeviceSlates.batch_picked_torch)


@pytest.fixture
def draws(monkeypatch):
    """counts FixLength's draws as the product makes them: {"choice": calls of :70, "rule": calls of :74 (the only one from an array)}"""
    from allrank_amd import data as ED
    counts = {"choice": 0, "rule": 0}
    orig = ED.reference_picks

    class Spy(object):
        def __init__(self, rng):
            self.rng = rng

        def choice(self, a, *args, **kw):
            counts["choice" if np.isscalar(a) else "rule"] += 1
            return self.rng.choice(a, *args, **kw)
    monkeypatch.setattr(ED, "reference_picks", lambda y, n, rng: orig(y, n, Spy(rng)))
    return counts


def _device_loaders(path, W, batch_size=8, rank=0, world=1):
    from allrank_amd import data as ED
    tr, va = ED.load_libsvm_dataset(path, L, "vali", device="cpu")
    return (ED.DeviceLoader(tr, world * batch_size, shuffle=True, rank=rank, world=world, sampling="reference", num_workers=W),
            ED.DeviceLoader(va, world * batch_size, shuffle=False, rank=rank, world=world, sampling="reference", num_workers=W))


def _states():
    return torch.get_rng_state(), np.random.get_state()


def _same_states(a, b):
    assert torch.equal(a[0], b[0]), "torch's global generator"
    assert a[1][0] == b[1][0] and np.array_equal(a[1][1], b[1][1]) and a[1][2:] == b[1][2:], "numpy's global generator"


@pytest.mark.parametrize("W", WORKERS)
def test_reference_sampling_equals_the_host_loader_bit_for_bit(tmp_path, torch_assembly, draws, W):
    path = write_sampled_job(tmp_path)
    _seed()
    ref = _epochs(*LO.create_data_loaders(*LO.load_libsvm_dataset(path, L, "vali"), num_workers=W, batch_size=8), n=2)
    ref_state = _states()
    _seed()
    tr, va = _device_loaders(path, W)
    assert tr.sampling == va.sampling == "reference" and tr.num_workers == W
    mine = _epochs(tr, va, n=2)
    _same_states(_states(), ref_state)
    _same(ref, mine)                                        # x, y, indices; no canonical re-ordering
    sampled = sum(int((b[2] >= 0).all(1).sum()) for b in mine)
    assert sampled > 0 and draws["rule"] > 0                # both are exercised ...
    assert draws["choice"] > sampled                        # ... and so is the repeated draw (more draws than sampled rows)
    # the rule's signature in the output: a sampled row of slate 20 whose LAST slot holds the slate's only relevant item
    assert any(bool(((b[1].sum(1) == 1) & (b[2][:, -1] == 41) & (b[2] >= 0).all(1)).any()) for b in mine if b[2].shape[1] == L)


@pytest.mark.parametrize("W", WORKERS)
def test_burn_keeps_the_passes_that_are_made_on_the_reference_s_draws(tmp_path, torch_assembly, W):
    from allrank_amd import fit as EF
    path = write_sampled_job(tmp_path)
    _seed()
    tr_h, va_h = LO.create_data_loaders(*LO.load_libsvm_dataset(path, L, "vali"), num_workers=W, batch_size=8)
    ref = []
    for _ in range(2):                                      # the reference's traffic; only the first train / first val pass is kept
        ref += [tuple(t.clone() for t in b) for b in tr_h]
        list(tr_h)
        ref += [tuple(t.clone() for t in b) for b in va_h]
        list(va_h)
    ref_state = _states()
    _seed()
    tr, va = _device_loaders(path, W)
    mine = []
    for _ in range(2):
        mine += list(tr)
        assert EF._burn(tr)
        mine += list(va)
        assert EF._burn(va)
    _same_states(_states(), ref_state)
    _same(ref, mine)


@pytest.mark.parametrize("W", (0, 1))
def test_rank_blocks_concatenate_to_the_one_rank_batch(tmp_path, torch_assembly, W):
    from allrank_amd.data import ShardBatch
    path = write_sampled_job(tmp_path)
    for world in (2, 3):
        _seed()
        one = _epochs(*_device_loaders(path, W, 4 * world), n=1, extra_train=0, extra_val=0)
        one_state = _states()
        per_rank = []
        for r in range(world):
            _seed()                                         # every rank seeds identically (main.py:36-38)
            tr, va = _device_loaders(path, W, 4, rank=r, world=world)
            per_rank.append(list(tr) + list(va))
            _same_states(_states(), one_state)              # every rank made the whole global batch's draws
        assert all(len(p) == len(one) for p in per_rank)
        assert any(bool((whole[2] >= 0).all(1).any()) for whole in one)
        for k, whole in enumerate(one):
            blocks = [p[k] for p in per_rank]
            assert all(isinstance(b, ShardBatch) and b.global_slates == whole[0].shape[0] for b in blocks)
            for j in range(3):
                assert torch.equal(torch.cat([b[j] for b in blocks]), whole[j])


@pytest.mark.parametrize("W", (0, 1))
def test_id_batches_yield_the_slates_of_iter_and_leave_the_same_generator_states(tmp_path, torch_assembly, W):
    path = write_sampled_job(tmp_path)
    for which in (0, 1):                                    # the training loader (sampled to L) and the validation loader (packable)
        _seed()
        dl = _device_loaders(path, W)[which]
        full = list(dl)
        after_iter = _states()
        _seed()
        ids = list(dl.id_batches())
        _same_states(_states(), after_iter)
        assert len(ids) == len(full)
        s = dl.dataset.slates
        for b, i in zip(full, ids):
            assert (b.order_tag, b.global_slates, b.offset) == (i.order_tag, i.global_slates, i.offset)
            assert torch.equal(b.lengths, i.lengths)
            # stored order: the rows of __iter__ as SETS (sampled rows: a subset of the slate's stored items)
            stored = s.batch_picked_torch(i.ids, s.longest_query_length, torch.full((len(i.ids),), -1, dtype=torch.int32))
            for r in range(len(i.ids)):
                keep = b[2][r][b[2][r] >= 0]
                assert torch.equal(stored[0][r][keep], b[0][r][b[2][r] >= 0]) and torch.equal(stored[1][r][keep], b[1][r][b[2][r] >= 0])


def test_environment_switch(tmp_path, torch_assembly, monkeypatch):
    from allrank_amd import data as ED
    path = write_sampled_job(tmp_path)
    monkeypatch.delenv("ALLRANK_AMD_SAMPLING", raising=False)
    tr, va = ED.load_libsvm_dataset(path, L, "vali", device="cpu")
    a, b = ED.create_data_loaders(tr, va, num_workers=1, batch_size=8)
    assert a.sampling == b.sampling == tr.sampling == "device" and a.num_workers == 0
    assert ED.DeviceLoader(tr, 8).sampling == "device"
    monkeypatch.setenv("ALLRANK_AMD_SAMPLING", "reference")
    tr, va = ED.load_libsvm_dataset(path, L, "vali", device="cpu")
    a, b = ED.create_data_loaders(tr, va, num_workers=1, batch_size=8)
    assert a.sampling == b.sampling == tr.sampling == "reference" and a.num_workers == b.num_workers == 1 and a.shuffle and not b.shuffle
    # ... and the loaders it builds are the reference's
    _seed()
    ref = _epochs(*LO.create_data_loaders(*LO.load_libsvm_dataset(path, L, "vali"), num_workers=1, batch_size=8), n=1)
    _seed()
    _same(ref, _epochs(a, b, n=1))
    # ds[i] draws from numpy's global generator like the reference's __getitem__
    host = LO.load_libsvm_dataset(path, L, "vali")[0]
    for i in (20, 5, 0):
        _seed()
        want = host[i]
        st = np.random.get_state()[1].copy()
        _seed()
        got = tr[i]
        assert all(torch.equal(u, v) for u, v in zip(want, got)) and np.array_equal(np.random.get_state()[1], st)
    monkeypatch.setenv("ALLRANK_AMD_SAMPLING", "exact")
    with pytest.raises(ValueError, match="'device' or 'reference'"):
        ED.create_data_loaders(tr, va, num_workers=1, batch_size=8)
    with pytest.raises(ValueError, match="'device' or 'reference'"):
        ED.DeviceLoader(tr, 8, sampling="host")


@pytest.mark.skipif(not reference_available(), reason="needs a checkout of allegro/allRank (ALLRANK_REFERENCE)")
def test_committed_sampled_trajectory_equals_the_live_reference():
    """the drift guard of tests/test_golden_drift.py for tests/golden/trajectory_sampled_golden.npz: integers identical, floats to 1e-6"""
    state = torch.get_rng_state(), np.random.get_state()
    try:
        built = importlib.import_module("tests.golden.make_golden_trajectory_sampled").build()
    finally:
        torch.set_rng_state(state[0])
        np.random.set_state(state[1])
    (fname, fresh), = built.items()
    committed = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", fname))
    assert set(committed.files) == set(fresh), sorted(set(committed.files) ^ set(fresh))[:10]
    for k in committed.files:
        a, b = np.asarray(committed[k]), np.asarray(fresh[k])
        assert a.shape == b.shape and a.dtype.kind == b.dtype.kind, (k, a.shape, b.shape, a.dtype, b.dtype)
        if a.dtype.kind in "iub":
            assert np.array_equal(a, b), k
        elif a.dtype.kind in "US":
            assert (a == b).all(), k
        else:
            assert np.isfinite(a).all() and np.isfinite(b).all(), k
            a64, b64 = a.astype(np.float64), b.astype(np.float64)
            assert float((np.abs(a64 - b64) / (1.0 + np.abs(a64))).max(initial=0.0)) <= 1e-6, k
