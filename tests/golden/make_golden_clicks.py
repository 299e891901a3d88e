"""Generate tests/golden/click_golden.npz from the REAL reference on CPU: for every case of tests/click_cases.py, what the reference's own
``click_on_slates(..., include_empty=True)`` (allrank/click_models/click_utils.py:10-27) returns under ``np.random.seed(case seed)``.

Stored per case: X and y; the uniforms consumed (re-drawn from the same seed); the clicks; the duplicate margins, as ``np.quantile`` of
scipy's ``cdist`` in fp64 (0 for a slate without a pair or a model that is not diverse); the numpy generator's state afterwards (its sha256: click_cases.state_digest).

GAP CONDITION (asserted here for the "gauss" cases): every distance a greedy comparison uses differs from the margin by more than
1e-9 x the margin, unless it EQUALS the margin -- the margin's own pair, for an odd pair count.  A click that differs from the stored
one is then a bug, not rounding; the case seeds are chosen so that the assertion holds.

    python tests/golden/make_golden_clicks.py        # build container only
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle.ref_loader import load_reference  # noqa: E402
from tests import click_cases as CC  # noqa: E402


def _margins(model, X, y):
    from scipy.spatial.distance import cdist
    dm = CC.margin_model(model)
    out = np.zeros(X.shape[0], dtype=np.float64)
    if dm is None:
        return out
    for b in range(X.shape[0]):
        rows = X[b][y[b] != -1]
        if rows.shape[0] > 1:
            d = cdist(rows, rows, metric="euclidean")
            out[b] = np.quantile(d[np.triu_indices(rows.shape[0], 1)], q=dm[1])
    return out


def build():
    load_reference()
    from allrank.click_models.click_utils import click_on_slates
    out = {}
    state = np.random.get_state()
    try:
        for name, c in CC.CASES.items():
            X, y = CC.inputs(name)
            np.random.seed(c["seed"])
            _, clicks = click_on_slates((torch.tensor(X), torch.tensor(y)), CC.theirs(c["model"]), include_empty=True)
            after = np.random.get_state()
            clicks = np.stack([np.asarray(v) for v in clicks]).astype(np.float32)
            assert clicks.shape == y.shape, (name, clicks.shape)
            if c["kind"] == "gauss":
                used = []
                u = CC.uniforms(name)
                CC.restate_batch(c["model"], X, y, rand=_Replay(u), used=used)
                bad = CC.gap_violations(used)
                assert not bad, "make_golden_clicks: %s has %d comparisons within %g of the margin; pick another seed" % (name, len(bad), CC.GAP)
            out[name + ".X"], out[name + ".y"] = X, y
            out[name + ".u"] = CC.uniforms(name)
            out[name + ".clicks"] = clicks
            out[name + ".margin"] = _margins(c["model"], X, y)
            out[name + ".state"] = np.asarray(CC.state_digest(after))
    finally:
        np.random.set_state(state)
    return {"click_golden.npz": out}


class _Replay(object):
    """hands out a recorded stream of uniforms the way np.random.rand(n) does"""

    def __init__(self, u):
        self.u, self.at = u, 0

    def __call__(self, n):
        self.at += n
        return self.u[self.at - n:self.at]


def main():
    for f, d in build().items():
        np.savez_compressed(os.path.join(HERE, f), **d)
        print(f, os.path.getsize(os.path.join(HERE, f)), "bytes")


if __name__ == "__main__":
    main()
