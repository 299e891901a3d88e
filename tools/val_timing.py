"""One validation pass at the reference's validation shape, three ways: the nn.Module forward over the padded batches (what
``fit`` runs for validation slates longer than the training slates), and the packed scorer (engine.FusedScorer) eager and
captured -- plus ``ragged``: the captured scorer with the loss and the metrics on the packed rows as well
(fit(val_scorer="ragged"), allrank_amd.ragged) -- and one ``fit()`` epoch of a WEB30K-fold-sized job with each scorer.

    python tools/val_timing.py [--models c3,nn96] [--batches 64,256] [--reps 3] [--paths module,captured,ragged] [--epoch]
                               [--only PATH] [--json OUT]

Set: a WEB30K-vali-shaped set of 6,306 slates, lengths round(lognormal(ln 100, 0.6)) clipped to [1, 1251] (bench.py's
``_web30k_lengths``), 136 features on the 4-decimal grid of [0, 1), labels ~ Cat(.52, .32, .13, .02, .01), resident in HBM and read
through ``DeviceLoader`` padded to its longest slate (dataset_loading.py:185-194).  Models: BASELINE config 3 (fc[512], 2 x
self-attention d512 h8 d_ff 2048) and the neuralndcg_web30k shape (fc[96], 2 x self-attention d96 h1 d_ff 384, fixed positional
encoding), freshly initialised; validation loss ApproxNDCG, metrics NDCG@5, @10.  The three paths run interleaved in one process,
after one warm-up pass each, through ``fit._evaluate`` itself (so the outputs compared are the ones fit() reports).  ``--only``
runs a single path once (for a kernel trace of it under rocprofv3).  ``--epoch``: two epochs of ``fit()`` (18.9 k training
slates at slate_length 240, the validation set above), per scorer; the second epoch is reported.
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

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench import _web30k_lengths  # noqa: E402

DEV = "cuda:0"
F = 136
MODELS = {
    "c3": dict(fc=[512], N=2, h=8, d_ff=2048, pe=None),
    "nn96": dict(fc=[96], N=2, h=1, d_ff=384, pe=dict(strategy="fixed", max_indices=1260)),
}


def make_slates(n, seed):
    from allrank_amd.data import DeviceSlates
    lens = _web30k_lengths(n, 1251, seed)
    rng = np.random.default_rng(seed)
    m = int(lens.sum())
    X = (rng.integers(0, 10000, size=(m, F), dtype=np.int32) / np.float32(10000)).astype(np.float32)
    y = rng.choice(5, size=m, p=[0.52, 0.32, 0.13, 0.02, 0.01]).astype(np.float32)
    q = np.repeat(np.arange(n), lens)
    return DeviceSlates(X, y, q, device=DEV), lens


def make_model(spec, seed=7):
    from allrank_amd.model import make_model as mk
    torch.manual_seed(seed)
    return mk(dict(sizes=spec["fc"], input_norm=False, activation=None, dropout=0.0),
              dict(N=spec["N"], d_ff=spec["d_ff"], h=spec["h"], positional_encoding=spec["pe"], dropout=0.1),
              dict(d_output=1, output_activation=None), F).to(DEV)


def arithmetic(spec, lens, B):
    """rows and forward FLOP of one pass: padded (module) vs packed"""
    d, dff, N = spec["fc"][-1], spec["d_ff"], spec["N"]
    per_row = 2 * F * d + N * (2 * d * 3 * d + 2 * d * d + 2 * 2 * d * dff) + 2 * d
    Lv = int(lens.max())
    nb = -(-len(lens) // B)
    padded_rows = nb * B * Lv
    valid_rows = int(lens.sum())
    att_padded = N * nb * B * 4.0 * Lv * Lv * d                       # QK^T and PV, every head, padded grid
    att_packed = N * 4.0 * float((lens.astype(np.float64) ** 2).sum()) * d
    return dict(padded_rows=padded_rows, valid_rows=valid_rows, proj_flop_per_row=per_row,
                module_tflop=(padded_rows * per_row + att_padded) / 1e12, packed_tflop=(valid_rows * per_row + att_packed) / 1e12)


def one_pass(path, model, ft, loader, scorers, loss, metrics):
    from allrank_amd import fit as EF
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if path == "module":
        model.eval()
        vl, vm = EF._evaluate(model, loss, loader, DEV, metrics)
    elif path == "ragged":
        vl, vm = EF._evaluate(model, loss, loader, DEV, metrics, ft, 1, 0, scorers[path], EF._ragged_plan(loss, ft, metrics))
    else:
        vl, vm = EF._evaluate(model, loss, loader, DEV, metrics, ft, 1, 0, scorers[path])
    torch.cuda.synchronize()
    return time.perf_counter() - t0, float(vl), {k: float(v) for k, v in vm.items()}


def time_pass(args, slates, lens):
    from allrank_amd import data as ED, losses as E
    from allrank_amd.engine import FusedTrainer
    rows = []
    loss, metrics = partial(E.approxNDCGLoss), {"ndcg": [5, 10]}
    paths = [args.only] if args.only else args.paths.split(",")
    for name in args.models.split(","):
        spec = MODELS[name]
        for B in [int(b) for b in args.batches.split(",")]:
            model = make_model(spec)
            ft = FusedTrainer(model, "approxNDCGLoss", {}, B, 240, lr=1e-3, use_graph=True)
            loader = ED.DeviceLoader(ED.DeviceLibSVMDataset(slates), B, shuffle=False)
            Lv = loader.slate_length
            cap = {Lv: ft.scorer(B, Lv)}
            scorers = {"eager": {Lv: ft.scorer(B, Lv, use_graph=False)}, "captured": cap, "ragged": cap}
            res = {p: [] for p in paths}
            out = {}
            reps = 1 if args.only else args.reps + 1                       # (first round: warm-up, graph captures)
            for r in range(reps):
                for p in paths:
                    t, vl, vm = one_pass(p, model, ft, loader, scorers, loss, metrics)
                    if r > 0 or args.only:
                        res[p].append(t)
                    out[p] = dict(val_loss=vl, **vm)
            row = dict(model=name, B=B, L_val=Lv, times_s={p: res[p] for p in paths},
                       median_s={p: float(np.median(res[p])) for p in paths}, outputs=out,
                       scorer_bytes=scorers["captured"][Lv].nbytes, graphs=sorted(scorers["captured"][Lv]._graphs),
                       arithmetic=arithmetic(spec, lens, B))
            print(json.dumps(row), flush=True)
            rows.append(row)
            del model, ft, scorers
            torch.cuda.empty_cache()
    return rows


def time_epoch(args, val_slates):
    from allrank_amd import data as ED, fit as EF, losses as E
    tr_slates, tr_lens = make_slates(18900, 11)
    out = []
    for scorer in args.scorers.split(","):
        for B in [int(b) for b in args.batches.split(",")]:
            torch.manual_seed(42)
            np.random.seed(42)
            tr = ED.DeviceLibSVMDataset(tr_slates, 240)
            va = ED.DeviceLibSVMDataset(val_slates)
            model = make_model(MODELS["c3"])
            opt = torch.optim.Adam(model.parameters(), lr=1e-3)
            cfg = types.SimpleNamespace(metrics={"ndcg": [5, 10]}, val_metric="ndcg_5")
            res = EF.fit(epochs=2, model=model, loss_func=partial(E.approxNDCGLoss), optimizer=opt, scheduler=None,
                   train_dl=ED.DeviceLoader(tr, B, shuffle=True), valid_dl=ED.DeviceLoader(va, B, shuffle=False), config=cfg,
                   gradient_clipping_norm=None, early_stopping_patience=100, device=torch.device(DEV),
                   output_dir=tempfile.mkdtemp(), tensorboard_output_path=None, val_scorer=scorer)
            ep = EF.last_run["epoch_log"][-1]
            items = float(np.minimum(tr_lens, 240).sum())
            row = dict(scorer=EF.last_run["val_scorer"], B=B, train_s=ep["train_s"], val_s=ep["val_s"], val_loss=ep["val_loss"],
                       train_items_per_s=items / ep["train_s"], epoch_items_per_s=items / (ep["train_s"] + ep["val_s"]),
                       val_loss_per_epoch=[e["val_loss"] for e in EF.last_run["epoch_log"]],
                       train_metrics={k: float(v) for k, v in res["train_metrics"].items()})
            print(json.dumps(row), flush=True)
            out.append(row)
            del model, opt
            torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="c3,nn96")
    ap.add_argument("--batches", default="64,256")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--paths", default="module,eager,captured,ragged", help="the interleaved paths of the pass timing, in order")
    ap.add_argument("--only", choices=["module", "eager", "captured", "ragged"])
    ap.add_argument("--epoch", action="store_true")
    ap.add_argument("--scorers", default="module,packed", help="validation scorers of the --epoch runs, in order")
    ap.add_argument("--no-pass", action="store_true", help="skip the validation-pass timing (with --epoch)")
    ap.add_argument("--json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("val_timing.py measures on the GPU; none is visible")
    slates, lens = make_slates(6306, 12)
    print(json.dumps(dict(slates=len(lens), longest=int(lens.max()), valid_items=int(lens.sum()))), flush=True)
    res = dict(passes=[] if args.no_pass else time_pass(args, slates, lens))
    if args.epoch:
        res["epochs"] = time_epoch(args, slates)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
