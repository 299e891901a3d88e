"""-m gpu: ``DeviceLoader(sampling="reference")`` through the real kernels (``ltrx_assemble_batch_picked`` behind the device parse):
the job of tests/test_sampling_cpu.py -- both relevance branches of FixLength's sampling (dataset_loading.py:61-79) -- against the
restated host loader of the reference (oracle/loader_oracle.py), same seeds: every batch of two epochs of the reference's loader
traffic bit for bit (``x``, ``y``, ``indices``, sampled order included), torch's and numpy's global generators in the same state
afterwards, for ``num_workers`` 0 and 1; and the rank blocks of world 2 == the one-rank batches."""
import pytest
import torch

from oracle import loader_oracle as LO
from tests.test_loader_cpu import _seed, _epochs, _same
from tests.test_sampling_cpu import L, write_sampled_job, _states, _same_states

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _device_loaders(path, W, batch_size=8, rank=0, world=1):
    from allrank_amd import data as ED
    tr, va = ED.load_libsvm_dataset(path, L, "vali", device=DEV)
    return (ED.DeviceLoader(tr, world * batch_size, shuffle=True, rank=rank, world=world, sampling="reference", num_workers=W),
            ED.DeviceLoader(va, world * batch_size, shuffle=False, rank=rank, world=world, sampling="reference", num_workers=W))


@pytest.mark.parametrize("W", [0, 1])
def test_reference_sampling_equals_the_host_loader_bit_for_bit(tmp_path, W):
    path = write_sampled_job(tmp_path)
    _seed()
    ref = _epochs(*LO.create_data_loaders(*LO.load_libsvm_dataset(path, L, "vali"), num_workers=W, batch_size=8), n=2)
    ref_state = _states()
    _seed()
    mine = _epochs(*_device_loaders(path, W), n=2)
    _same_states(_states(), ref_state)
    assert all(t.is_cuda for b in mine for t in b)
    _same(ref, mine)
    assert sum(int((b[2] >= 0).all(1).sum()) for b in mine) > 0
    assert any(bool(((b[1].sum(1) == 1) & (b[2][:, -1] == 41) & (b[2] >= 0).all(1)).any()) for b in mine if b[2].shape[1] == L)


def test_rank_blocks_concatenate_to_the_one_rank_batch(tmp_path):
    path = write_sampled_job(tmp_path)
    _seed()
    one = _epochs(*_device_loaders(path, 1, 8), n=1, extra_train=0, extra_val=0)
    per_rank = []
    for r in range(2):
        _seed()
        per_rank.append([b for dl in _device_loaders(path, 1, 4, rank=r, world=2) for b in dl])
    assert len(per_rank[0]) == len(per_rank[1]) == len(one)
    for k, whole in enumerate(one):
        for j in range(3):
            assert torch.equal(torch.cat([per_rank[0][k][j], per_rank[1][k][j]]), whole[j])
