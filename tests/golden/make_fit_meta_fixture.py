"""Record the job-description block the autograd engine writes into a checkpoint (``checkpoint.make_meta``) for three small CPU jobs.

    python tests/golden/make_fit_meta_fixture.py [--out FILE]

tests/golden/fit_job_meta_parent.json was recorded ONCE, at the parent of the change that moved the autograd halves of fit.py's
checkpoint helpers next to ``engine.Trainer``: there the block came from ``fit._job_meta(None, False, model, loss_func, optimizer,
clip)``, which this script still calls where it exists; at any later commit it is ``Trainer.meta()``, and tests/test_fit_stats_cpu.py
holds that to the recorded value.  Re-running the script at a later commit only re-records that commit against itself.
"""
import functools
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIXTURE = os.path.join(HERE, "fit_job_meta_parent.json")


def _plain_loss(y_pred, y_true):
    return ((y_pred - y_true) ** 2).mean()


def jobs():
    """{name: (model, loss_func, optimizer, gradient_clipping_norm)} -- Adam and SGD in the neutral schema with a bound loss, and a
    class the schema does not cover with a plain function as the loss"""
    from allrank_amd import losses as E
    from allrank_amd.model import make_model

    def model():
        torch.manual_seed(3)
        return make_model(dict(sizes=[16], input_norm=False, activation=None, dropout=0.0),
                          dict(N=1, d_ff=32, h=2, positional_encoding=None, dropout=0.1), dict(d_output=1, output_activation=None), 12)
    a, s, r = model(), model(), model()
    return {
        "adam": (a, functools.partial(E.approxNDCGLoss, alpha=2.0), torch.optim.Adam(a.parameters(), lr=2e-3, betas=(0.8, 0.99), eps=1e-7,
                                                                                       weight_decay=0.01), None),
        "sgd": (s, functools.partial(E.listNet, 1e-9), torch.optim.SGD(s.parameters(), lr=0.05, momentum=0.9, nesterov=True), 1.5),
        "rmsprop": (r, _plain_loss, torch.optim.RMSprop(r.parameters(), lr=1e-3, alpha=0.9), None),
    }


def meta_of(model, loss_func, optimizer, clip):
    from allrank_amd import fit as EF
    from allrank_amd.engine import Trainer
    if hasattr(EF, "_job_meta"):
        return EF._job_meta(None, False, model, loss_func, optimizer, clip)
    return Trainer(model, loss_func, optimizer, clip).meta()


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else FIXTURE
    with open(out, "w") as fh:
        json.dump({name: meta_of(*job) for name, job in jobs().items()}, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote %s" % out)


if __name__ == "__main__":
    main()
