"""Generate tests/golden/trajectory_sampled_golden.npz from the REAL reference (allegro/allRank) on CPU: the training trajectory of
``allrank.main.run()`` (main.py:34-110; its own fit, loaders, losses, metrics, torch.optim.Adam) on ONE job whose training slates go
through FixLength's SAMPLING branch (dataset_loading.py:61-79) -- what tests/golden/make_golden_trajectory.py's jobs never do -- so
that ``DeviceLoader(sampling="reference")`` + ``allrank_amd.fit.fit`` can be held to the reference's own draws on the GPU box.

The job (dropout 0, seeds 42 as main.py:36-38 sets them): ragged slates of 5..48 items, ``slate_length`` 32 (about 4 training slates
in 10 are sampled), six long training slates with exactly one relevant item (the "keep the only relevant item" rule, :72-74),
validation slates of up to 48 items (padded to their longest, whose holders are permuted by the sampling branch in every pass),
FC[32] + 2 encoder layers (h 2, d_ff 64) + ApproxNDCG, ndcg@5/@10, 3 epochs.  It runs twice: ``num_workers`` 1 (the value every shipped
config has: the draws come from the worker's generator) and 0 (numpy's global generator).

Recorded: the data, the config, the initial weights, and per run and epoch: the ``indices`` tensor of every training batch in order,
training / validation loss and metrics, the weights after the epoch; how often the single-relevant rule fired in the main process of
the ``num_workers`` 0 run.  Hooks wrap ``loss_batch`` / ``compute_metrics`` / ``epoch_summary`` of the imported package in memory; nothing
of the reference is modified or copied.

    python tests/golden/make_golden_trajectory_sampled.py        # build container only
"""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle.ref_loader import load_reference  # noqa: E402
from tests.golden.make_golden_trajectory import write_job_files  # noqa: E402

NAME = "ragged_sampled_approx"
WORKERS = (1, 0)
SLATE_LENGTH = 32
CONFIG = {
    "model": {"fc_model": {"sizes": [32], "input_norm": False, "activation": None, "dropout": 0.0},
              "transformer": {"N": 2, "d_ff": 64, "h": 2, "positional_encoding": None, "dropout": 0.0},
              "post_model": {"output_activation": None, "d_output": 1}},
    "data": {"path": None, "validation_ds_role": "vali", "num_workers": 1, "batch_size": 16, "slate_length": SLATE_LENGTH},
    "optimizer": {"name": "Adam", "args": {"lr": 0.001}},
    "lr_scheduler": {"name": None, "args": {}},
    "training": {"epochs": 3, "early_stopping_patience": 100, "gradient_clipping_norm": None},
    "val_metric": "ndcg_5", "metrics": ["ndcg_5", "ndcg_10"],
    "loss": {"name": "approxNDCGLoss", "args": {}},
    "expected_metrics": {"val": {"ndcg_5": 0.0}},
}


def job_data():
    """{role: (X f32, y f32, qid i64)}"""
    rng = np.random.default_rng(11)
    out = {}
    for role, n_q in (("train", 96), ("vali", 32)):
        lens = rng.integers(5, 49, n_q)
        if role == "train":
            lens[[4, 17, 30, 43, 56, 69]] = 48
        X = rng.standard_normal((lens.sum(), 16)).astype(np.float32)
        y = rng.choice(5, size=lens.sum(), p=[0.5, 0.25, 0.15, 0.06, 0.04]).astype(np.float32)
        if role == "train":
            starts = np.concatenate([[0], np.cumsum(lens)])
            for q in (4, 17, 30, 43, 56, 69):                    # exactly one relevant item among 48
                y[starts[q]:starts[q + 1]] = 0
                y[starts[q] + int(rng.integers(0, 48))] = 1
        out[role] = (X, y, np.repeat(np.arange(2000, 2000 + n_q), lens).astype(np.int64))
    lens = np.bincount(out["train"][2] - 2000)
    assert 4 * (lens >= SLATE_LENGTH).sum() >= len(lens) and lens.max() > SLATE_LENGTH
    assert np.bincount(out["vali"][2] - 2000).max() > SLATE_LENGTH
    return out


def _run_reference(cfg, data, tmp):
    import allrank.main as M
    import allrank.training.train_utils as TU
    folder = os.path.join(tmp, "data")
    write_job_files(data, folder)
    cfg = json.loads(json.dumps(cfg))
    cfg["data"]["path"] = folder
    cfg_path = os.path.join(tmp, "cfg.json")
    with open(cfg_path, "w") as fh:
        json.dump(cfg, fh)
    rec = {"indices": [], "epochs": [], "weights": [], "init": None, "rule": 0}
    cur = {"indices": [], "n_metric_calls": 0}
    orig_lb, orig_cm, orig_es, orig_choice = TU.loss_batch, TU.compute_metrics, TU.epoch_summary, np.random.choice

    def loss_batch(model, loss_func, xb, yb, indices, gradient_clipping_norm, opt=None):
        if opt is not None:
            if rec["init"] is None:
                rec["init"] = {k: v.detach().clone().numpy() for k, v in model.state_dict().items()}
            cur["indices"].append(indices.detach().cpu().numpy().astype(np.int16))
        return orig_lb(model, loss_func, xb, yb, indices, gradient_clipping_norm, opt)

    def compute_metrics(metrics, model, dl, dev):
        out = orig_cm(metrics, model, dl, dev)
        cur["n_metric_calls"] += 1
        if cur["n_metric_calls"] % 2 == 1:                       # train_utils.py:99 (train), :107 (validation)
            cur["train_metrics"] = dict(out)
        else:
            cur["val_metrics"] = dict(out)
            rec["weights"].append({k: v.detach().clone().numpy() for k, v in model.state_dict().items()})
        return out

    def epoch_summary(epoch, train_loss, val_loss, train_metrics, val_metrics):
        rec["epochs"].append((float(train_loss), float(val_loss), dict(cur["train_metrics"]), dict(cur["val_metrics"])))
        rec["indices"].append(list(cur["indices"]))
        cur["indices"] = []
        return orig_es(epoch, train_loss, val_loss, train_metrics, val_metrics)

    def choice(a, *args, **kw):                                  # (main process only: what a num_workers = 0 run draws)
        rec["rule"] += int(not np.isscalar(a))                   # :74 is the one call that samples from an ARRAY
        return orig_choice(a, *args, **kw)

    TU.loss_batch, TU.compute_metrics, TU.epoch_summary, np.random.choice = loss_batch, compute_metrics, epoch_summary, choice
    old_argv = sys.argv
    sys.argv = ["allrank", "--job-dir", os.path.join(tmp, "job"), "--run-id", "traj", "--config-file-name", cfg_path]
    try:
        M.run()                                                  # main.py:34-110, the reference's own fit
    finally:
        sys.argv = old_argv
        TU.loss_batch, TU.compute_metrics, TU.epoch_summary, np.random.choice = orig_lb, orig_cm, orig_es, orig_choice
    return rec


def build():
    import logging
    load_reference(stable_sort=True)
    data = job_data()
    names = list(CONFIG["metrics"])
    out = {"job": np.array(NAME), "workers": np.array(WORKERS, dtype=np.int64), "metric_names": np.array(names)}
    for role, (X, y, qid) in data.items():
        out["data/%s/X" % role], out["data/%s/y" % role], out["data/%s/qid" % role] = X, y, qid
    for W in WORKERS:
        cfg = json.loads(json.dumps(CONFIG))
        cfg["data"]["num_workers"] = W
        with tempfile.TemporaryDirectory() as tmp:
            rec = _run_reference(cfg, data, tmp)
        for h in list(logging.getLogger("allrank").handlers):    # (init_logger adds a file handler per run)
            logging.getLogger("allrank").removeHandler(h)
        p = "w%d/" % W
        out[p + "config"] = np.array(json.dumps(cfg))
        out[p + "train_loss"] = np.array([e[0] for e in rec["epochs"]], dtype=np.float64)
        out[p + "val_loss"] = np.array([e[1] for e in rec["epochs"]], dtype=np.float64)
        out[p + "train_metrics"] = np.array([[float(e[2][m]) for m in names] for e in rec["epochs"]], dtype=np.float64)
        out[p + "val_metrics"] = np.array([[float(e[3][m]) for m in names] for e in rec["epochs"]], dtype=np.float64)
        for e, batches in enumerate(rec["indices"]):
            out[p + "indices_epoch%d" % e] = np.concatenate(batches)       # [n_slates, L]; batches are 16 rows each, the last shorter
            out[p + "batch_sizes_epoch%d" % e] = np.array([len(b) for b in batches], dtype=np.int64)
        if "init/" + next(iter(rec["init"])) not in out:                   # the same for both runs (checked below)
            for k, v in rec["init"].items():
                out["init/" + k] = v
        assert all(np.array_equal(out["init/" + k], v) for k, v in rec["init"].items())
        for e, wts in enumerate(rec["weights"]):
            for k, v in wts.items():
                out[p + "weights_epoch%d/%s" % (e, k)] = v
        if W == 0:
            assert rec["rule"] > 0, "the single-relevant rule never fired: pick other data"
            out["w0/single_relevant_rule_fired"] = np.array(rec["rule"], dtype=np.int64)
    return {"trajectory_sampled_golden.npz": out}


if __name__ == "__main__":
    for fname, arrays in build().items():
        np.savez_compressed(os.path.join(HERE, fname), **arrays)
        print("wrote", fname, len(arrays), "arrays", os.path.getsize(os.path.join(HERE, fname)), "bytes")
