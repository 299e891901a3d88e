"""The SHARDED form of the fused step at 46 input features, on a one-rank ``nccl`` group (``FusedTrainer(force_dist=True)``, as
tests/rccl_one_rank_worker.py runs it at 24): a one-rank sum is the identity, so losses, gradients and weights must equal the
non-distributed step's bit for bit, captured and eager, with and without ``input_norm`` -- and the flat layout and its gradient
buckets are the ones the same model has without sharding.

    odd_features_dist_worker.py
"""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from allrank_amd.engine import FusedTrainer  # noqa: E402
from allrank_amd.model import make_model  # noqa: E402

F, B, L = 46, 4, 16


def build(norm):
    torch.manual_seed(7)
    return make_model(dict(sizes=[32], input_norm=norm, activation=None, dropout=0.0),
                      dict(N=1, d_ff=64, h=4, positional_encoding=None, dropout=0.0), dict(d_output=1, output_activation=None), F).to("cuda:0")


def main():
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29534")
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    rng = np.random.default_rng(3)
    x = torch.tensor(rng.standard_normal((B, L, F)).astype(np.float32), device=dev)
    y = torch.tensor(rng.integers(0, 5, (B, L)).astype(np.float32), device=dev)
    for b, n in enumerate([16, 9, 1, 13]):
        y[b, n:] = -1
        x[b, n:] = 0
    for norm in (False, True):
        plain = FusedTrainer(build(norm), "approxNDCGLoss", {}, B, L, lr=1e-3, use_graph=True)
        cap = FusedTrainer(build(norm), "approxNDCGLoss", {}, B, L, lr=1e-3, world_size=1, use_graph=True, force_dist=True)
        eag = FusedTrainer(build(norm), "approxNDCGLoss", {}, B, L, lr=1e-3, world_size=1, use_graph=False, force_dist=True)
        assert cap.sharded and eag.sharded and not plain.sharded and cap._x_pad and cap._x_stride == 48
        assert cap._buckets == plain._buckets and cap.nflat == plain.nflat
        assert [r.off for r in cap.params] == [r.off for r in plain.params]
        for step in range(5):                                     # two eager warm-ups, the capture step, two replays
            lp, lc, le = (tr.step(x, y).clone() for tr in (plain, cap, eag))
            assert torch.isfinite(lp).all() and torch.equal(lp, lc) and torch.equal(lp, le), (norm, step, "loss")
            assert torch.equal(plain.flat_g, cap.flat_g) and torch.equal(plain.flat_g, eag.flat_g), (norm, step, "gradients")
            assert torch.equal(plain.flat_p, cap.flat_p) and torch.equal(plain.flat_p, eag.flat_p), (norm, step, "weights")
        assert cap.capture_fallback is None and cap.graph is not None and len(cap.graph) >= 1 + len(cap._buckets)
    torch.cuda.synchronize()
    dist.destroy_process_group()
    print("ODD_FEATURES_DIST_OK")


if __name__ == "__main__":
    main()
