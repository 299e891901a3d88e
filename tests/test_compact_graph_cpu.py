"""The host-side rules of FusedTrainer(compact="graph") -- no GPU: the per-bucket warm-up and key rule of engine._GraphLRU (driven by a
fake capture, as tests/test_graph_lru_cpu.py drives it), fit()'s reading of ``compact`` / ALLRANK_AMD_COMPACT, and the trainer's row
bucket against ``row_bucket``."""
import pytest

from allrank_amd import fit as FIT
from allrank_amd.engine import FusedTrainer, _GraphLRU, row_bucket


class _Seg(object):
    def __init__(self, log, tag):
        self.log, self.tag = log, tag

    def replay(self):
        self.log.append(("replay", self.tag))


class _Fake(object):
    """the step cache of compact="graph": keys (batch divisor, collectives on?, rows), warm-up counted over the rows"""

    def __init__(self, max_graphs=8):
        self.log, self.evicted = [], []
        self.c = _GraphLRU(max_graphs, capture=self.capture, warm=lambda key: key[2], on_evict=self.evicted.append,
                           new_pool=object)

    def capture(self, fn):
        self.log.append(("capture", fn.tag))
        return [(_Seg(self.log, fn.tag), None)]

    def run(self, key):
        def eager():
            self.log.append(("eager", key))
        eager.tag = key
        return self.c.run(key, eager)


def test_warm_up_is_counted_per_row_bucket_and_a_new_divisor_in_a_warm_bucket_is_captured_at_once():
    f = _Fake()
    full = lambda rows: (6.0, True, rows)  # noqa: E731
    for rows in (192, 256, 288):                                    # every bucket: two eager visits of its own, then capture, replay
        assert [f.run(full(rows)) for _ in range(4)] == ["eager", "eager", "capture", "replay"], rows
    assert f.run((4.0, True, 256)) == "capture"                     # the short last batch of an epoch, in a bucket that is warm
    assert f.run((4.0, True, 256)) == "replay" and f.run(full(256)) == "replay"
    assert f.run((4.0, True, 320)) == "eager"                       # ... and in one that is not: the bucket's own warm-up
    assert [f.run((6.0, True, 320)), f.run((6.0, True, 320)), f.run((4.0, True, 320))] == ["eager", "capture", "capture"]
    # interleaved visits: the count is per bucket, whatever comes between
    g = _Fake()
    seq = [32, 64, 32, 64, 32, 64, 32, 64]
    assert [g.run((6.0, True, r)) for r in seq] == ["eager", "eager", "eager", "eager", "capture", "capture", "replay", "replay"]
    # collectives on / off is part of the key, not of the warm-up slot
    assert g.run((6.0, False, 32)) == "capture"


def test_clearing_the_captures_keeps_the_warm_up_counts_and_the_bound_is_the_lru_bound():
    f = _Fake(max_graphs=2)
    keys = [(6.0, True, r) for r in (32, 64, 96)]
    for k in keys:
        assert [f.run(k) for _ in range(3)] == ["eager", "eager", "capture"]
    assert list(f.c.graphs) == keys[1:] and f.evicted == [keys[0]] and f.c.evictions == 1
    f.c.graphs.clear()                                              # what set_lr does
    assert [f.run(k) for k in keys] == ["capture"] * 3              # no new eager visits
    assert ("eager", keys[0]) not in f.log[-6:]


def test_the_named_warm_up_policies_are_unchanged():
    for warm, second in (("key", "eager"), ("cache", "capture")):
        f = _Fake()
        f.c = _GraphLRU(4, capture=f.capture, warm=warm)
        assert [f.run("a") for _ in range(3)] == ["eager", "eager", "capture"]
        assert f.run("b") == second
    with pytest.raises(KeyError):
        _GraphLRU(4, capture=lambda fn: [], warm="bucket")


def test_compact_argument_and_environment_variable(monkeypatch):
    monkeypatch.delenv("ALLRANK_AMD_COMPACT", raising=False)
    assert FIT._compact_mode(None) is None and FIT._compact_mode(True) is True and FIT._compact_mode(False) is False
    assert FIT._compact_mode(0) is False and FIT._compact_mode("graph") == "graph" and FIT._compact_mode("GRAPH") == "graph"
    with pytest.raises(ValueError, match="compact"):
        FIT._compact_mode("packed")
    monkeypatch.setenv("ALLRANK_AMD_COMPACT", "graph")
    assert FIT._compact_mode(None) == "graph"
    assert FIT._compact_mode(False) is False and FIT._compact_mode(True) is True       # an explicit argument wins
    monkeypatch.setenv("ALLRANK_AMD_COMPACT", "")
    assert FIT._compact_mode(None) is None
    for bad in ("1", "true", "eager", "graphs"):
        monkeypatch.setenv("ALLRANK_AMD_COMPACT", bad)
        with pytest.raises(ValueError, match="ALLRANK_AMD_COMPACT"):
            FIT._compact_mode(None)


def test_stats_of_a_trainer_without_the_mode_are_none():
    class T(object):
        compact_graph = False
    assert FIT._compact_graph_stats(T()) is None and FIT._compact_graph_stats(object()) is None


@pytest.mark.parametrize("B,L", [(6, 70), (5, 70), (64, 240), (1, 7)])
def test_the_trainers_bucket_is_row_bucket_capped_at_the_allocation(B, L):
    class T(object):
        bucket_of = FusedTrainer.bucket_of
    t = T()
    t.cap = (B * L + 31) // 32 * 32                                 # what the constructor allocates in this mode
    counts = [0, 1, 31, 32, 33, 255, 256, 257, 288, 289, B * L - 1, B * L]
    counts = [n for n in counts if n <= B * L]
    got = t.bucket_of(counts)
    assert got == [row_bucket(max(n, 1), t.cap) for n in counts]
    for n, r in zip(counts, got):
        assert r % 32 == 0 and max(n, 1) <= r <= t.cap, (n, r)
        assert r - n <= max(32, r // 8), (n, r)                     # alignment rows: at most 31 below 256, 1/8 of the bucket above
