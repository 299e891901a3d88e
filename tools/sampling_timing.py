"""What ``DeviceLoader(sampling="reference")`` costs against the default ``sampling="device"``: the reference's FixLength draws are made
on the host, batch by batch (allrank_amd/data.py), while the GPU runs the previous step -- does the host work hide?

    python tools/sampling_timing.py [--batches 64,256] [--rounds 2] [--epochs 3] [--json OUT]

Set: tools/val_timing.py's WEB30K-shaped generator -- 18,900 training slates, lengths round(lognormal(ln 100, 0.6)) clipped to
[1, 1251], 136 features -- resident in HBM, ``slate_length`` 240 (about 7 % of the slates are sampled); a 256-slate validation set
of at most 240 items (the validation pass is not what is measured).  Model: BASELINE config 3 (fc[512], 2 x self-attention d512 h8
d_ff 2048), ApproxNDCG.  Measured, the two modes interleaved in one process:
  * ``fit()``: per mode ``rounds`` calls of 1 + ``epochs`` epochs (the first epoch of a call is the warm-up: graph capture, host label
    download), alternating device, reference, device, ...; valid items/s of every timed training pass (``last_run["epoch_log"]``);
  * the loader alone: one pass over the training loader, nothing consuming the batches;
  * the kernels: ``ltrx_assemble_batch_picked`` against ``ltrx_fixlength_positions`` + ``ltrx_assemble_batch`` on the same batch.
"""
import argparse
import json
import os
import sys
import tempfile
import time
import types
from functools import partial

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench import _web30k_lengths  # noqa: E402
from val_timing import DEV, F, MODELS, make_model, make_slates  # noqa: E402

L = 240
MODES = (("device", 0), ("reference", 1))


def small_val_set(n=256, seed=5):
    from allrank_amd.data import DeviceSlates
    lens = _web30k_lengths(n, L, seed)
    rng = np.random.default_rng(seed)
    m = int(lens.sum())
    X = (rng.integers(0, 10000, size=(m, F), dtype=np.int32) / np.float32(10000)).astype(np.float32)
    y = rng.choice(5, size=m, p=[0.52, 0.32, 0.13, 0.02, 0.01]).astype(np.float32)
    return DeviceSlates(X, y, np.repeat(np.arange(n), lens), device=DEV)


def loaders(tr_slates, va_slates, B, mode, W):
    from allrank_amd import data as ED
    return (ED.DeviceLoader(ED.DeviceLibSVMDataset(tr_slates, L), B, shuffle=True, sampling=mode, num_workers=W),
            ED.DeviceLoader(ED.DeviceLibSVMDataset(va_slates), B, shuffle=False, sampling=mode, num_workers=W))


def fit_epochs(tr_slates, va_slates, B, mode, W, epochs):
    """seconds of every training pass after the warm-up epoch"""
    from allrank_amd import fit as EF, losses as E
    torch.manual_seed(42)
    np.random.seed(42)
    tr, va = loaders(tr_slates, va_slates, B, mode, W)
    model = make_model(MODELS["c3"])
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    cfg = types.SimpleNamespace(metrics={"ndcg": [5, 10]}, val_metric="ndcg_5")
    EF.fit(epochs=1 + epochs, model=model, loss_func=partial(E.approxNDCGLoss), optimizer=opt, scheduler=None, train_dl=tr, valid_dl=va,
           config=cfg, gradient_clipping_norm=None, early_stopping_patience=100, device=torch.device(DEV), output_dir=tempfile.mkdtemp(),
           tensorboard_output_path=None)
    assert EF.last_run["engine"] == "fused" and EF.last_run["sampling"] == mode, EF.last_run
    out = [e["train_s"] for e in EF.last_run["epoch_log"][1:]]
    del model, opt
    torch.cuda.empty_cache()
    return out


def loader_pass(tr_slates, va_slates, B, mode, W):
    tr, _ = loaders(tr_slates, va_slates, B, mode, W)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in tr:
        pass
    host = time.perf_counter() - t0                     # the host is done issuing
    torch.cuda.synchronize()
    return host, time.perf_counter() - t0


def kernel_times(tr_slates, lens, B, reps=50):
    """microseconds per batch: (one launch from picks, the two launches it replaces) on the same B slates"""
    rng = np.random.default_rng(3)
    ids = rng.permutation(len(lens))[:B]
    slates = torch.from_numpy(ids).to(DEV)
    pos = tr_slates.positions(slates, L, 99)
    long_rows = np.flatnonzero(lens[ids] >= L)
    pick_row = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    pick_row[torch.from_numpy(long_rows).to(DEV)] = torch.arange(len(long_rows), dtype=torch.int32, device=DEV)
    picks = pos[torch.from_numpy(long_rows).to(DEV)].to(torch.int32).contiguous()
    out = []
    for fn in (lambda: tr_slates.batch_picked(slates, L, pick_row, picks), lambda: tr_slates.batch(slates, L, seed=99)):
        for _ in range(5):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1000.0 / reps)
    return out[0], out[1], int(len(long_rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="64,256")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sampling_timing.py measures on the GPU; none is visible")
    tr_slates, lens = make_slates(18900, 11)
    va_slates = small_val_set()
    items = float(np.minimum(lens, L).sum())
    head = dict(slates=len(lens), sampled_slates=int((lens >= L).sum()), valid_items=items, L=L)
    print(json.dumps(head), flush=True)
    rows = []
    for B in [int(b) for b in args.batches.split(",")]:
        t_host = time.perf_counter()
        tr_slates._host_labels.clear()
        tr_slates.host_labels(L)
        t_labels = time.perf_counter() - t_host
        res = {m: [] for m, _ in MODES}
        for _ in range(args.rounds):
            for mode, W in MODES:
                res[mode] += fit_epochs(tr_slates, va_slates, B, mode, W, args.epochs)
        lp = {m: [] for m, _ in MODES}
        for _ in range(3):
            for mode, W in MODES:
                lp[mode].append(loader_pass(tr_slates, va_slates, B, mode, W))
        k_new, k_old, n_long = kernel_times(tr_slates, lens, B)
        med = {m: float(np.median(res[m])) for m in res}
        row = dict(B=B, train_s=res, median_train_s=med, items_per_s={m: items / med[m] for m in med},
                   reference_vs_device=med["device"] / med["reference"],
                   loader_only_s={m: dict(host=float(np.median([h for h, _ in lp[m]])), total=float(np.median([t for _, t in lp[m]]))) for m in lp},
                   host_labels_download_s=t_labels, kernel_us=dict(picked=k_new, positions_plus_assemble=k_old, sampled_rows=n_long))
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(dict(head, rows=rows), fh, indent=1)


if __name__ == "__main__":
    main()
