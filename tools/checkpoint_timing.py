"""What checkpointing costs, measured through fit() itself at BASELINE configs[2] (bench.py's attn_approxndcg workload) with 256
slates of 240 items per batch, batches resident on the device:

    python tools/checkpoint_timing.py --mode off      # ms per training step with the feature off (epoch 0 = warm-up, left out)
    python tools/checkpoint_timing.py --mode on       # ... and with checkpoint_every=1: ckpt_s per write, the file's size

``--mode off`` passes fit() nothing new, so ``--tree <older checkout>`` runs the same command against an older tree for an A/B of the step time.
Every epoch's ``train_s`` ends in the epoch's one host sync, so train_s / steps is a step time.  Prints one JSON line."""
import argparse
import json
import os
import sys
import tempfile
import types
from functools import partial

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Batches(object):
    """``steps`` device-resident batches per pass, cycling over a few distinct ones"""

    def __init__(self, batches, steps):
        self.batches, self.steps = batches, steps

    def __len__(self):
        return self.steps

    def __iter__(self):
        for k in range(self.steps):
            yield self.batches[k % len(self.batches)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["off", "on"], default="on")
    ap.add_argument("--slates", type=int, default=256)
    ap.add_argument("--steps", type=int, default=24, help="training steps per epoch")
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--tree", default=ROOT, help="the checkout whose allrank_amd and bench.py are measured (A/B against an older one)")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import bench
    import allrank_amd
    from allrank_amd import fit as EF, losses as E
    dev = torch.device("cuda:0")
    w = bench.WORKLOADS["attn_approxndcg"]
    L = 240
    model = bench.build_model(w, dev)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=50, gamma=0.1)
    train = Batches([bench.synth_batch(a.slates, L, w["n_features"], 100 + k, dev) for k in range(4)], a.steps)
    valid = Batches([bench.synth_batch(a.slates, L, w["n_features"], 200, dev)], 1)
    cfg = types.SimpleNamespace(metrics={"ndcg": [5]}, val_metric="ndcg_5")
    with tempfile.TemporaryDirectory() as out:
        kw = dict(checkpoint_every=1) if a.mode == "on" else {}
        EF.fit(epochs=a.epochs, model=model, loss_func=partial(getattr(E, w["loss"])), optimizer=opt, scheduler=sched, train_dl=train,
               valid_dl=valid, config=cfg, gradient_clipping_norm=None, early_stopping_patience=100, device=dev, output_dir=out,
               tensorboard_output_path=None, compact=False, **kw)
        run = EF.last_run
        size = os.path.getsize(os.path.join(out, "checkpoint.pt")) if a.mode == "on" else None
    log = run["epoch_log"][1:]
    print(json.dumps({"tree": os.path.dirname(os.path.abspath(allrank_amd.__file__)), "mode": a.mode, "engine": run["engine"],
                      "slates": a.slates, "steps_per_epoch": a.steps, "params": sum(p.numel() for p in model.parameters()),
                      "step_ms": [round(1e3 * e["train_s"] / a.steps, 4) for e in log],
                      "train_s": [round(e["train_s"], 4) for e in log],
                      "ckpt_s": [round(e["ckpt_s"], 4) for e in log] if a.mode == "on" else None, "file_bytes": size}))


if __name__ == "__main__":
    main()
