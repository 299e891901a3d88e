"""Shared by tests/test_rank_cpu.py and tests/test_gpu_rank.py: the golden ranking fixture (tests/golden/make_golden_rank.py) as an
allrank_amd model, a dataset in the reference's item form and a config."""
import os
import types

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rank_golden.npz")


class HostSlates(torch.utils.data.Dataset):
    """what a reference LibSVMDataset item is after its transforms: (x [L, F] f32, y [L] f32, indices [L] i64), on the host"""

    def __init__(self, x, y):
        self.x, self.y = torch.as_tensor(x), torch.as_tensor(y)

    def __len__(self):
        return self.x.shape[0]

    def __getitem__(self, i):
        return self.x[i], self.y[i], torch.arange(self.x.shape[1])


def config(batch_size):
    return types.SimpleNamespace(data=types.SimpleNamespace(batch_size=int(batch_size), num_workers=0))


def golden():
    return dict(np.load(GOLDEN, allow_pickle=False))


def golden_model(g, device):
    from allrank_amd.model import make_model
    tr = dict(N=int(g["cfg.N"]), d_ff=int(g["cfg.d_ff"]), h=int(g["cfg.h"]),
              positional_encoding=dict(strategy="fixed", max_indices=int(g["cfg.max_indices"])), dropout=0.0)
    model = make_model(dict(sizes=[int(v) for v in g["cfg.fc_sizes"]], input_norm=False, activation=None, dropout=0.0), tr,
                       dict(d_output=1, output_activation=None), int(g["cfg.n_features"]))
    sd = {k.split(".", 1)[1]: torch.tensor(v) for k, v in g.items() if k.startswith(("param.", "buffer."))}
    model.load_state_dict(sd)
    return model.to(device)
