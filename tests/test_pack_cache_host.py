"""functional.PackCache on CPU tensors with a counting ``make``: the one freshness rule of every packed-weight cache (same
objects, versions, addresses, weights epoch), alias resolution, sweeping of dead entries, and the entries() / restamp() pair
that the batched repack uses.  No GPU, no library."""
import gc

import pytest
import torch

from druggen_amd import functional as dgf
from druggen_amd.functional import _runtime


class Make:
    """``make`` of a cache: a copy of the weights' sum (so that content can be compared), counting its calls."""

    def __init__(self):
        self.calls = 0

    def __call__(self, *weights):
        self.calls += 1
        return sum(w.detach().clone() for w in weights)


def _w(seed, n=4):
    return torch.full((n,), float(seed))


def test_second_get_returns_the_same_object_without_make():
    cache, make, w = dgf.PackCache(16), Make(), _w(1)
    p = cache.get((w,), (0,), make)
    assert cache.get((w,), (0,), make) is p and make.calls == 1
    assert torch.equal(p, w) and len(cache) == 1


@pytest.mark.parametrize("change", ["inplace", "epoch", "data"])
def test_each_change_alone_causes_exactly_one_remake(change):
    cache, make, w = dgf.PackCache(16), Make(), _w(1)
    p = cache.get((w,), (), make)
    if change == "inplace":
        w.add_(1)
    elif change == "epoch":
        dgf.bump_weights_epoch()
    else:
        before = w._version
        w.data = w.detach().clone()      # the address moves; the version counter does not
        assert w._version == before
    q = cache.get((w,), (), make)
    assert q is not p and make.calls == 2
    assert torch.equal(q, w)
    assert cache.get((w,), (), make) is q and make.calls == 2
    assert len(cache) == 1


@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("change", ["inplace", "data"])
def test_three_weight_entry_remakes_when_any_one_weight_changes(which, change):
    cache, make, ws = dgf.PackCache(16), Make(), (_w(1), _w(2), _w(3))
    p = cache.get(ws, (0,), make)
    assert cache.get(ws, (0,), make) is p and make.calls == 1
    if change == "inplace":
        ws[which].mul_(2)
    else:
        ws[which].data = ws[which].detach().clone()
    q = cache.get(ws, (0,), make)
    assert q is not p and make.calls == 2 and torch.equal(q, ws[0] + ws[1] + ws[2])
    assert cache.get(ws, (0,), make) is q and make.calls == 2


def test_distinct_extra_and_distinct_weight_order_are_distinct_entries():
    cache, make, a, b = dgf.PackCache(16), Make(), _w(1), _w(2)
    p0 = cache.get((a,), (0, torch.float32), make)
    p1 = cache.get((a,), (1, torch.float32), make)
    p2 = cache.get((a,), (0, torch.bfloat16), make)
    assert make.calls == 3 and len({id(p0), id(p1), id(p2)}) == 3
    assert cache.get((a,), (1, torch.float32), make) is p1
    ab, ba = cache.get((a, b), (), make), cache.get((b, a), (), make)
    assert ab is not ba and make.calls == 5 and len(cache) == 5
    # keys as the tests of the row-GEMM packs evict them: (ids of the weights..., extra...)
    assert cache.pop((id(a), 1, torch.float32)) is p1
    assert cache.pop((id(a), 1, torch.float32)) is None and len(cache) == 4
    assert cache.get((a,), (1, torch.float32), make) is not p1 and make.calls == 6


def test_alias_of_a_parameter_hits_the_parameters_entry():
    cache, make, w = dgf.PackCache(16), Make(), _w(1)
    p = cache.get((w,), (0,), make)
    alias = dgf._weight_alias(w)
    assert alias is not w and dgf._canon(alias) is w
    assert cache.get((alias,), (0,), make) is p and make.calls == 1 and len(cache) == 1
    # the other way round: the alias asks first, the entry made is the parameter's
    v = _w(2)
    q = cache.get((dgf._weight_alias(v),), (0,), make)
    assert cache.get((v,), (0,), make) is q and make.calls == 2


def test_alias_does_not_resolve_to_a_stale_entry_after_its_parameter_changed():
    cache, make, w = dgf.PackCache(16), Make(), _w(1)
    alias = dgf._weight_alias(w)
    p = cache.get((alias,), (), make)
    w.add_(1)      # (a view shares its base's version counter: both move)
    q = cache.get((alias,), (), make)
    assert q is not p and make.calls == 2 and torch.equal(q, w)
    # the parameter is given new storage: the alias still shows the old one and no longer stands for the parameter
    w.data = torch.full((4,), 7.0)
    assert dgf._canon(alias) is alias
    r = cache.get((alias,), (), make)
    assert make.calls == 3 and torch.equal(r, alias) and not torch.equal(r, w)
    s = cache.get((w,), (), make)
    assert make.calls == 4 and torch.equal(s, w)


def test_inserting_past_the_limit_removes_exactly_the_dead_entries():
    cache, make = dgf.PackCache(4), Make()
    live = [_w(i) for i in range(3)]
    dead = [_w(10 + i) for i in range(3)]
    pair_mate = _w(20)
    packs = [cache.get((w,), (), make) for w in live + dead]
    cache.get((live[0], pair_mate), (), make)      # an entry with ONE dead weight goes as well
    assert len(cache) == 7
    live_keys = {(id(w),) for w in live}
    del dead, pair_mate
    gc.collect()
    assert len(cache) == 7                          # nothing happens until an insert finds the cache over its limit
    extra = _w(30)      # (may get a dead weight's id and so replace its entry: the count below holds either way)
    cache.get((extra,), (), make)
    assert {k for k, *_ in cache.entries()} == live_keys | {(id(extra),)} and len(cache) == 4
    for w, p in zip(live, packs):
        assert cache.get((w,), (), make) is p
    assert make.calls == 8


def test_a_cache_under_its_limit_is_not_swept_by_an_insert():
    cache, make = dgf.PackCache(16), Make()
    w, v = _w(1), _w(2)      # (both exist before either dies: a new tensor may get a dead one's id, and with it its key)
    cache.get((w,), (), make)
    del w
    gc.collect()
    cache.get((v,), (), make)
    del v
    gc.collect()
    assert len(cache) == 2 and cache.entries() == []
    cache.sweep()
    assert len(cache) == 0


def test_epoch_bump_past_its_threshold_sweeps_every_registered_cache(monkeypatch):
    a, b, make = dgf.PackCache(1 << 20), dgf.PackCache(1 << 20), Make()
    assert a in _runtime._pack_caches and b in _runtime._pack_caches
    keep_a, keep_b = _w(1), _w(2)
    a.get((keep_a,), (), make)
    b.get((keep_b,), (), make)
    doomed = [_w(i) for i in range(10)]
    for i in range(5):
        a.get((doomed[i],), (), make)
        b.get((doomed[5 + i],), (), make)
    del doomed
    gc.collect()
    assert len(a) == 6 and len(b) == 6
    others = sum(len(c) for c in _runtime._pack_caches) - len(a) - len(b)
    monkeypatch.setattr(_runtime, "_EPOCH_SWEEP_ABOVE", others + len(a) + len(b))
    dgf.bump_weights_epoch()             # at the threshold: no sweep
    assert len(a) > 1 and len(b) > 1
    monkeypatch.setattr(_runtime, "_EPOCH_SWEEP_ABOVE", others + len(a) + len(b) - 1)
    dgf.bump_weights_epoch()
    assert [k for k, *_ in a.entries()] == [(id(keep_a),)] and len(a) == 1
    assert [k for k, *_ in b.entries()] == [(id(keep_b),)] and len(b) == 1


def test_entries_lists_live_entries_with_their_named_parts_and_skips_dead_weights():
    cache, make = dgf.PackCache(16), Make()
    a, b, c = _w(1), _w(2), _w(3)
    pa = cache.get((a,), (0, torch.float32), make)
    pbc = cache.get((b, c), (1,), make)
    gone, gone2 = _w(4), _w(5)
    cache.get((gone,), (0, torch.float32), make)
    cache.get((a, gone2), (), make)
    del gone, gone2
    gc.collect()
    got = {key: (ws, extra, packed, ptrs) for key, ws, extra, packed, ptrs in cache.entries()}
    assert set(got) == {(id(a), 0, torch.float32), (id(b), id(c), 1)}
    ws, extra, packed, ptrs = got[(id(a), 0, torch.float32)]
    assert ws[0] is a and len(ws) == 1 and extra == (0, torch.float32) and packed is pa and ptrs == (a.data_ptr(),)
    ws, extra, packed, ptrs = got[(id(b), id(c), 1)]
    assert ws[0] is b and ws[1] is c and extra == (1,) and packed is pbc and ptrs == (b.data_ptr(), c.data_ptr())
    assert len(cache) == 4                               # entries() itself removes nothing


@pytest.mark.parametrize("change", ["inplace", "epoch"])
def test_restamp_turns_a_stale_entry_into_a_hit_without_make(change):
    cache, make, ws = dgf.PackCache(16), Make(), (_w(1), _w(2))
    p = cache.get(ws, (0,), make)
    if change == "inplace":
        ws[1].add_(1)
    else:
        dgf.bump_weights_epoch()
    (key, _, _, packed, _), = cache.entries()
    packed.copy_(ws[0] + ws[1])      # what the batched repack does: the same storage, refreshed from the weights as they are
    cache.restamp(key)
    assert cache.get(ws, (0,), make) is p and make.calls == 1 and torch.equal(p, ws[0] + ws[1])
    ws[0].add_(1)                    # and the refreshed entry goes stale like any other
    assert cache.get(ws, (0,), make) is not p and make.calls == 2
    cache.restamp(("no", "such", "key"))      # (an entry evicted in the meantime: nothing to do)
