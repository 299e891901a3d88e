"""Generate tests/golden/scale_golden.npz from the REAL reference (CPU, build container only):
    python tests/golden/make_golden_scale.py
The slates of tests/cases.py SCALE_SETS with their scores multiplied by SCALES = {1, 8, 30, 100, 1000}: a model in training emits
scores of |s| ~ 30 within a few steps, where the clamp and eps branches of the listwise losses decide the result (approxNDCG's
sigmoid saturates, lambdaLoss's max(sigmoid, eps) / max(q^w, eps), log(P + eps) of listNet, log(C + eps) of listMLE, a near one-hot
NeuralSort matrix in NeuralNDCG).  Exact ties survive the multiplication.  Records the reference's fp32 loss and its autograd gradient
w.r.t. y_pred, NDCG / DCG at {1, 5, 10, L} with the stable order, and MRR at {1, 10}.  Sorts run with stable=True; listMLE's
torch.randperm is replaced by the recorded permutation (as in make_golden.py)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle.ref_loader import load_reference  # noqa: E402
from tests.cases import SCALES, SCALE_SETS, SCALE_NDCG_ATS, SCALE_MRR_ATS, scale_inputs, scale_loss_cases  # noqa: E402


def ref_loss(fn, s, y, **kw):
    sp = torch.tensor(s, requires_grad=True)
    loss = fn(sp, torch.tensor(y), **kw)
    if loss.requires_grad:
        loss.backward()
        g = sp.grad.numpy().copy()
    else:
        g = np.zeros_like(s)
    return np.float32(loss.item()), g


def build():
    load_reference(stable_sort=True)
    from allrank.models import losses as RL, metrics as RM
    fns = dict(listnet=RL.listNet, approxndcg=RL.approxNDCGLoss, lambdaloss=RL.lambdaLoss, ranknet=RL.rankNet,
               binary_listnet=RL.binary_listNet)
    out = {"scales": np.asarray(SCALES, np.int64)}
    for name, B, L, seed, ties, full in SCALE_SETS:
        s0, y = scale_inputs(B, L, seed, ties, name)
        yb = np.where(y == -1, -1, (y >= 2).astype(np.float32)).astype(np.float32)
        perm = np.random.default_rng(seed + 100).permutation(L).astype(np.int64)
        out[name + ".y"], out[name + ".yb"], out[name + ".perm"] = y, yb, perm
        ats = list(SCALE_NDCG_ATS) + [L]
        for sc in SCALES:
            s = (s0 * np.float32(sc)).astype(np.float32)
            pre = "%s.x%d." % (name, sc)
            out[pre + "s"] = s
            for cname, kind, kw in scale_loss_cases(full):
                key = pre + cname
                if kind == "listmle":
                    orig = torch.randperm
                    torch.randperm = lambda n, _p=perm: torch.tensor(_p)
                    try:
                        out[key + ".loss"], out[key + ".grad"] = ref_loss(RL.listMLE, s, y)
                    finally:
                        torch.randperm = orig
                elif kind == "neuralndcg":
                    kw = dict(kw)
                    fn = RL.neuralNDCG_transposed if kw.pop("transposed") else RL.neuralNDCG
                    out[key + ".loss"], out[key + ".grad"] = ref_loss(fn, s, y, **kw)
                else:
                    out[key + ".loss"], out[key + ".grad"] = ref_loss(fns[kind], s, yb if kind == "binary_listnet" else y, **kw)
            st, yt = torch.tensor(s), torch.tensor(y)
            out[pre + "ndcg"] = RM.ndcg(st, yt, ats=ats).numpy()
            out[pre + "dcg"] = RM.dcg(st, yt, ats=ats).numpy()
            out[pre + "mrr"] = RM.mrr(st, yt, ats=list(SCALE_MRR_ATS)).numpy()
            sm = st.clone()
            sm[yt == -1] = float("-inf")
            out[pre + "order"] = sm.sort(descending=True, dim=-1)[1].numpy().astype(np.int64)
    return {"scale_golden.npz": out}


def main():
    for f, d in build().items():
        np.savez_compressed(os.path.join(HERE, f), **d)
        print(f, os.path.getsize(os.path.join(HERE, f)), "bytes")


if __name__ == "__main__":
    main()
