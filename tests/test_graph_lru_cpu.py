"""The capture-and-replay rule of engine._GraphLRU -- LRU order and bound, the two warm-up policies, a failing capture, the
pool rule -- driven by a fake capture callable and a fake pool factory, so no GPU (and nothing of torch.cuda) is involved."""
import pytest

from allrank_amd.engine import _GraphLRU


class _Seg(object):
    """stands in for one hipGraph segment"""

    def __init__(self, log, tag):
        self.log, self.tag = log, tag

    def replay(self):
        self.log.append(("replay", self.tag))


class _Fake(object):
    """a cache whose captures are two fake segments with a host action between them, everything logged in call order"""

    def __init__(self, max_graphs, warm, fail=()):
        self.log, self.evicted, self.pools, self.fail, self.n = [], [], [], set(fail), 0
        self.c = _GraphLRU(max_graphs, capture=self.capture, warm=warm, on_evict=self.evicted.append, new_pool=self.new_pool)

    def new_pool(self):
        self.pools.append(object())
        return self.pools[-1]

    def capture(self, fn):
        tag = fn.tag
        if tag in self.fail:
            raise RuntimeError("capture of %r failed" % (tag,))
        self.log.append(("capture", tag, self.c.pool))
        return [(_Seg(self.log, tag), lambda: self.log.append(("after", tag))), (_Seg(self.log, tag), None)]

    def fn(self, tag):
        def eager():
            self.log.append(("eager", tag))
        eager.tag = tag
        return eager

    def run(self, key):
        return self.c.run(key, self.fn(key))

    def warm_up(self, key="w"):
        assert [self.run(key) for _ in range(3)] == ["eager", "eager", "capture"]


def test_lru_order_bound_and_eviction_callback():
    f = _Fake(3, "cache")
    f.warm_up("a")
    assert [f.run(k) for k in "bc"] == ["capture", "capture"]
    assert list(f.c.graphs) == ["a", "b", "c"] and f.c.evictions == 0 and f.evicted == []
    assert f.run("a") == "replay"                                   # a replay moves its key to the end ...
    assert list(f.c.graphs) == ["b", "c", "a"]
    assert f.run("d") == "capture"                                  # ... so the key beyond the bound evicts "b", not "a"
    assert list(f.c.graphs) == ["c", "a", "d"] and f.evicted == ["b"] and f.c.evictions == 1
    assert f.run("b") == "capture"                                  # an evicted key comes back by one re-capture
    assert list(f.c.graphs) == ["a", "d", "b"] and f.evicted == ["b", "c"] and f.c.evictions == 2
    assert len(f.c.graphs) == f.c.max_graphs == 3
    # a capture only records; the visit that captured and every replay run each segment, then its host action, in order
    f.log[:] = []
    assert f.run("d") == "replay"
    assert f.log == [("replay", "d"), ("after", "d"), ("replay", "d")]
    f.log[:] = []
    assert f.run("e") == "capture"
    assert [e[:2] for e in f.log] == [("capture", "e"), ("replay", "e"), ("after", "e"), ("replay", "e")]
    assert len(f.c.graphs["e"]) == 2                                # the captured object is the segment list


def test_warm_up_per_key():
    f = _Fake(4, "key")
    for key in ("a", "b", "c"):                                     # every new key: two eager visits of its own, then capture
        assert [f.run(key) for _ in range(4)] == ["eager", "eager", "capture", "replay"], key
    assert [e[:2] for e in f.log if e[1] == "b"] == [("eager", "b"), ("eager", "b"), ("capture", "b"), ("replay", "b"), ("after", "b"),
                                                     ("replay", "b"), ("replay", "b"), ("after", "b"), ("replay", "b")]
    assert _GraphLRU(4, capture=f.capture).run("z", f.fn("z")) == "eager"          # per key is the default


def test_warm_up_once_per_cache():
    f = _Fake(4, "cache")
    assert [f.run("a") for _ in range(4)] == ["eager", "eager", "capture", "replay"]
    for key in ("b", "c"):                                          # every later key is captured on its first visit
        assert [f.run(key) for _ in range(2)] == ["capture", "replay"], key
    g = _Fake(4, "cache")                                           # the two warm-up visits may be of different keys
    assert [g.run(k) for k in ("a", "b", "c", "a")] == ["eager", "eager", "capture", "capture"]


def test_capture_now_waits_for_the_warm_up_and_obeys_the_bound():
    f = _Fake(2, "cache")
    assert f.c.capture_now("a", f.fn("a")) is False and not f.c.graphs and f.log == [] and f.pools == []
    assert [f.run("a") for _ in range(2)] == ["eager", "eager"]
    f.log[:] = []
    assert f.c.capture_now("a", f.fn("a")) is True and list(f.c.graphs) == ["a"]
    assert [e[:2] for e in f.log] == [("capture", "a")]             # recorded, nothing executed
    assert f.c.capture_now("a", f.fn("a")) is True and len(f.log) == 1             # live: nothing to do
    assert f.run("a") == "replay" and f.run("b") == "capture"
    assert f.c.capture_now("c", f.fn("c")) is True
    assert list(f.c.graphs) == ["b", "c"] and f.evicted == ["a"] and len(f.c.graphs) == f.c.max_graphs
    p = _Fake(2, "key")                                             # per key: the warm-up of one key does nothing for another
    p.warm_up("a")
    assert p.c.capture_now("b", p.fn("b")) is False and list(p.c.graphs) == ["a"]


def test_a_raising_capture_leaves_no_entry_and_the_others_alone():
    f = _Fake(4, "cache", fail={"bad"})
    f.warm_up("a")
    assert f.run("b") == "capture"
    before = dict(f.c.graphs)
    for attempt in (lambda: f.run("bad"), lambda: f.c.capture_now("bad", f.fn("bad"))):
        with pytest.raises(RuntimeError, match="capture of 'bad' failed"):
            attempt()
        assert "bad" not in f.c.graphs and list(f.c.graphs) == ["a", "b"]
        assert all(f.c.graphs[k] is before[k] for k in before) and f.evicted == []
    assert ("eager", "bad") not in f.log                            # (the cache does not run eagerly on its own: the caller decides)
    assert f.run("a") == "replay" and f.run("b") == "replay"
    f.fail.clear()
    assert f.run("bad") == "capture"                                # no new warm-up once the capture works


def test_a_capture_into_an_empty_mapping_gets_a_fresh_pool():
    f = _Fake(2, "cache")
    assert f.pools == [] and f.c.pool is None                       # no pool before the first capture
    f.warm_up("a")
    assert f.run("b") == "capture"
    assert len(f.pools) == 1                                        # live captures share one pool
    assert [e[2] for e in f.log if e[0] == "capture"] == [f.pools[0]] * 2
    f.c.graphs.clear()                                              # emptied behind the cache's back, on the mapping itself
    assert f.run("a") == "capture" and f.run("b") == "capture"      # (no new warm-up either)
    assert len(f.pools) == 2 and f.pools[1] is not f.pools[0]
    assert [e[2] for e in f.log if e[0] == "capture"][2:] == [f.pools[1]] * 2
    one = _Fake(1, "cache")                                         # a bound of 1 evicts its way to an empty mapping: same rule
    one.warm_up("a")
    assert one.run("b") == "capture" and one.evicted == ["a"] and len(one.pools) == 2
    none = _GraphLRU(2, capture=f.capture)                          # without a pool factory the captures get pool None
    assert [none.run("k", f.fn("k")) for _ in range(3)][-1] == "capture" and none.pool is None
