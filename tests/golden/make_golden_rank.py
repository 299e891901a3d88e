"""Generate tests/golden/rank_golden.npz from the REAL reference on CPU: a small seeded encoder model with a fixed positional
encoding, padded slates, and what the reference's own ``rank_slates`` (allrank/inference/inference_utils.py:14-60) returns for
them through its own DataLoader -- two batches, so the concatenation is covered, and ``indices = ones`` (:47) is in the scores.

GAP CONDITION (asserted here): within every slate, adjacent reference scores of the valid items differ by at least
1e-3 * max(1, max|s|) -- 50 x the 2e-5 * max(1, max|s|) bar to which tests/test_gpu_packed_scorer.py holds the engine's scores against
the module's.  A ranking that differs from the stored one is then a bug, not rounding; SEED is chosen so that the assertion holds.

    python tests/golden/make_golden_rank.py        # build container only
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle.ref_loader import load_reference  # noqa: E402

SEED = 500
CFG = dict(n_features=20, fc_sizes=[32], N=1, d_ff=64, h=2, max_indices=30, batch_size=4)
LENS = [24, 3, 17, 1, 20, 9, 12]
L = 24
GAP = 1e-3


class _Slates(torch.utils.data.Dataset):
    """what a LibSVMDataset item is after its transforms: (x [L, F] f32, y [L] f32, indices [L] i64)"""

    def __init__(self, x, y):
        self.x, self.y = torch.tensor(x), torch.tensor(y)

    def __len__(self):
        return self.x.shape[0]

    def __getitem__(self, i):
        return self.x[i], self.y[i], torch.arange(self.x.shape[1])


def build():
    load_reference(stable_sort=True)
    from allrank.models.model import make_model
    from allrank.config import TransformerConfig, PositionalEncoding
    from allrank.inference.inference_utils import rank_slates

    torch.manual_seed(SEED)
    pe = PositionalEncoding(strategy="fixed", max_indices=CFG["max_indices"])
    tr = TransformerConfig(N=CFG["N"], d_ff=CFG["d_ff"], h=CFG["h"], positional_encoding=pe, dropout=0.0)
    model = make_model(dict(sizes=list(CFG["fc_sizes"]), input_norm=False, activation=None, dropout=0.0), tr,
                       dict(d_output=1, output_activation=None), CFG["n_features"])
    with torch.no_grad():
        for _, p_ in model.named_parameters():
            if p_.dim() == 1:
                p_.add_(0.1 * torch.randn_like(p_))
    rng = np.random.default_rng(SEED)
    n, F = len(LENS), CFG["n_features"]
    x = rng.standard_normal((n, L, F)).astype(np.float32)
    y = rng.integers(0, 5, (n, L)).astype(np.float32)
    for b, k in enumerate(LENS):
        x[b, k:], y[b, k:] = 0, -1
    config = types.SimpleNamespace(data=types.SimpleNamespace(batch_size=CFG["batch_size"], num_workers=0))
    ranked = rank_slates({"test": _Slates(x, y)}, model, config)
    X, Y = ranked["test"]

    # the gap condition, on the reference's own scores
    model.eval()
    with torch.no_grad():
        yt = torch.tensor(y)
        s = model.score(torch.tensor(x), yt == -1, torch.ones_like(yt).type(torch.long)).numpy()
    worst = np.inf
    for b, k in enumerate(LENS):
        if k > 1:
            worst = min(worst, float(np.diff(np.sort(s[b, :k])).min()) / max(1.0, float(np.abs(s[b, :k]).max())))
    assert worst >= GAP, "make_golden_rank: adjacent scores %.3g apart (relative); pick another SEED" % worst

    out = {"x": x, "y": y, "ranked_x": X.numpy(), "ranked_y": Y.numpy(), "scores": s.astype(np.float32),
           "dtype_x": np.asarray(str(X.dtype)), "dtype_y": np.asarray(str(Y.dtype)), "lens": np.asarray(LENS, dtype=np.int64),
           "min_gap": np.float64(GAP)}
    for k_, v_ in CFG.items():
        out["cfg." + k_] = np.asarray(v_)
    for n_, p_ in model.named_parameters():
        out["param." + n_] = p_.detach().numpy().copy()
    for n_, b_ in model.named_buffers():
        out["buffer." + n_] = b_.detach().numpy().copy()
    return {"rank_golden.npz": out}


def main():
    for f, d in build().items():
        np.savez_compressed(os.path.join(HERE, f), **d)
        print(f, os.path.getsize(os.path.join(HERE, f)), "bytes")


if __name__ == "__main__":
    main()
