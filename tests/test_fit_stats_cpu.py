"""fit.py's epoch statistics (``_EpochStats``) against a direct transcription of the two expressions the training pass and the
validation pass each wrote out before the accumulator existed -- values AND value types: ``python_float / np.float32`` and
``np.float32 / python_float`` promote differently, and ``make_result`` / the tensorboard writer see what comes out.  Also: the
job-description block of the autograd engine (``Trainer.meta()``) equals what ``fit._job_meta`` returned at the parent commit
(tests/golden/fit_job_meta_parent.json, tests/golden/make_fit_meta_fixture.py)."""
import json

import numpy as np
import pytest
import torch

from tests.golden import make_fit_meta_fixture as G

METRICS = {"ndcg": [5, 10], "mrr": [10]}


def _batches(seed, sizes, skip=()):
    """per batch: (loss share, slates of the global batch, this rank's slates, {metric: per-slate values [n, len(ats)]} -- a metric
    in ``skip`` is never accumulated, an empty shard (n = 0) brings no slates)"""
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand((), generator=g) * 3, n_glob, n, {name: torch.rand((n, len(ats)), generator=g) for name, ats in METRICS.items()
                                                          if name not in skip}) for n_glob, n in sizes]


def _parent_train(batches):
    """the training pass as fit() wrote it out: zeros for an empty shard, a metric never accumulated is left out"""
    tot, num = torch.zeros(()), 0
    tm = {name: None for name in METRICS}
    for share, n_glob, n, vals in batches:
        tot += share.detach().float().reshape(()) * n_glob
        num += n
        for name, v in vals.items():
            v = v.sum(0) if n > 0 else torch.zeros(len(METRICS[name]))
            tm[name] = v if tm[name] is None else tm[name] + v
    stats = torch.cat([tot.reshape(1), torch.tensor([float(num)])] + [tm[n].float() for n in METRICS if tm[n] is not None])
    stats = stats.cpu().numpy()
    n_all = max(stats[1], 1.0)
    train_loss = float(stats[0]) / n_all
    train_metrics, off = {}, 2
    for name, ats in METRICS.items():
        if tm[name] is None:
            continue
        for at in ats:
            train_metrics["%s_%d" % (name, at)] = float(stats[off]) / n_all
            off += 1
    return train_loss, train_metrics


def _parent_val(batches):
    """the validation pass as _evaluate wrote it out: an empty shard adds no metric, a metric without a sum is zero-filled"""
    tot, num = torch.zeros(()), 0
    acc = {name: None for name in METRICS}
    for share, n_glob, n, vals in batches:
        tot += share.detach().float().reshape(()) * n_glob
        num += n
        if n > 0:
            for name, v in vals.items():
                v = v.sum(0)
                acc[name] = v if acc[name] is None else acc[name] + v
    sums = [acc[name].float() if acc[name] is not None else torch.zeros(len(METRICS[name])) for name in METRICS]
    stats = torch.cat([tot.reshape(1), torch.tensor([float(num)])] + sums)
    stats = stats.cpu().numpy()
    n_all = max(float(stats[1]), 1.0)
    out, off = {}, 2
    for name, ats in METRICS.items():
        for at in ats:
            out["%s_%d" % (name, at)] = np.float32(stats[off] / n_all)
            off += 1
    return float(stats[0]) / n_all, out


def _ours(batches, train):
    """the same pass through the accumulator, finished as fit() (``train``) or ``_evaluate`` finishes it"""
    from allrank_amd import fit as EF
    stats = EF._EpochStats(METRICS, "cpu")
    for share, n_glob, n, vals in batches:
        stats.add(share.detach().float(), n_glob, n)
        for name, v in vals.items():
            if n > 0:
                stats.add_metric(name, v.sum(0))
            elif train:
                stats.add_metric(name, torch.zeros(len(METRICS[name])))
    loss_sum, n_slates, sums = stats.finish(1, zero_fill=not train)
    if train:
        n_all = max(n_slates, 1.0)
        return float(loss_sum) / n_all, {k: float(v) / n_all for k, v in sums.items()}
    n_all = max(float(n_slates), 1.0)
    return float(loss_sum) / n_all, {k: np.float32(v / n_all) for k, v in sums.items()}


def _same(got, want):
    assert type(got[0]) is type(want[0]) and got[0] == want[0], (got[0], want[0], type(got[0]), type(want[0]))
    assert list(got[1]) == list(want[1])
    for k in want[1]:
        assert type(got[1][k]) is type(want[1][k]) and got[1][k] == want[1][k], (k, got[1][k], want[1][k], type(got[1][k]), type(want[1][k]))


CASES = {
    "full_and_short_batches": dict(sizes=[(16, 16), (16, 16), (8, 8)]),
    "a_rank_of_two_with_an_empty_shard": dict(sizes=[(16, 8), (16, 8), (1, 0)]),
    "one_slate": dict(sizes=[(1, 1)]),                                # (max(np.float32(1), 1.0) keeps the numpy scalar)
    "every_shard_empty": dict(sizes=[(1, 0), (1, 0)]),                # a zero slate count: the divisor is 1.0
    "no_batch": dict(sizes=[]),
    "a_metric_never_accumulated": dict(sizes=[(16, 16), (8, 8)], skip=("ndcg",)),
    "no_metric_accumulated": dict(sizes=[(16, 16), (8, 8)], skip=("ndcg", "mrr")),
}


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("train", [True, False], ids=["train", "val"])
def test_epoch_stats_equal_the_parent_expressions_in_value_and_type(case, train):
    batches = _batches(5, **CASES[case])
    _same(_ours(batches, train), (_parent_train if train else _parent_val)(batches))


def test_layout_rules_omit_for_training_zero_fill_for_validation():
    batches = _batches(6, [(16, 16), (1, 0)], skip=("ndcg",))
    assert list(_ours(batches, True)[1]) == ["mrr_10"]
    val = _ours(batches, False)[1]
    assert list(val) == ["ndcg_5", "ndcg_10", "mrr_10"] and val["ndcg_5"] == 0.0 and val["mrr_10"] > 0.0
    # an empty shard's zeros: the layout of a rank that saw no slate at all is the layout of its peers
    empty = _ours(_batches(6, [(1, 0)]), True)
    assert list(empty[1]) == ["ndcg_5", "ndcg_10", "mrr_10"] and set(empty[1].values()) == {0.0}


def test_trainer_meta_equals_the_parents_job_meta():
    from allrank_amd.engine import Trainer
    with open(G.FIXTURE) as fh:
        want = json.load(fh)
    jobs = G.jobs()
    assert sorted(want) == sorted(jobs) == ["adam", "rmsprop", "sgd"]
    for name, (model, loss_func, optimizer, clip) in jobs.items():
        trainer = Trainer(model, loss_func, optimizer, clip)
        assert json.loads(json.dumps(trainer.meta())) == want[name], name
        # made once: a scheduler's edit of the learning rate does not reach the block a checkpoint is compared on
        optimizer.param_groups[0]["lr"] *= 0.5
        assert trainer.meta() == trainer.state_dict()["meta"] and json.loads(json.dumps(trainer.meta())) == want[name], name


def test_both_engines_offer_the_members_fit_uses():
    from allrank_amd.engine import FusedTrainer, Trainer
    for member in ("step_block", "score_block", "first_nonfinite", "scanned", "set_lr", "meta", "state_dict", "load_state_dict"):
        assert hasattr(Trainer, member) and hasattr(FusedTrainer, member), member
    assert (Trainer.compact, Trainer.compact_graph, Trainer.fcstep) == (False, False, False)
    assert (Trainer.scanned, FusedTrainer.scanned) == ("weight", "gradient")
