"""The host prioritised replay buffer (srl_amd/runtime/replay.py) against the REAL reference's segment trees and buffer bookkeeping
(tests/golden/replay.npz, written by tests/golden/gen_replay.py), bit for bit: every tree node after every assignment, every
``find_prefixsum_idx`` (masses exactly on leaf boundaries included), ``max_priority`` and the beta schedule; initial priorities and
importance weights to one float32 ulp.  Then the documented differences, validation, wrap-around and ``make_buffer``."""
import types

import numpy as np
import pytest

from srl_amd.api.trainer import SampleBatch
from srl_amd.namedarray import NamedArray
from srl_amd.runtime import buffer as buffer_mod
from srl_amd.runtime import replay
from srl_amd.runtime.replay import LinearScheduler, PrioritizedReplayBuffer


@pytest.fixture(scope="module")
def g(golden):
    return golden("replay.npz")


def ulp32(a, b):
    """Distance of two float32 arrays in units in the last place (both finite, same sign)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def make_sample(Tb, k, ret=None, value=None):
    """One actor's [Tb, ...] sample: a uint8 frame leaf, flags, a float32 reward, each filled with a value that names (k, t)."""
    t = np.arange(Tb)
    obs = np.broadcast_to(((k * 16 + t) % 256).astype(np.uint8)[:, None, None], (Tb, 3, 4)).copy()
    ar = None if ret is None else NamedArray(ret=ret, value=value)
    return SampleBatch(obs=NamedArray(obs=obs), on_reset=(t == 0).astype(np.uint8).reshape(Tb, 1), done=np.zeros((Tb, 1), np.uint8),
                       truncated=np.zeros((Tb, 1), np.uint8), reward=(k + t / 8.0).astype(np.float32).reshape(Tb, 1),
                       analyzed_result=ar)


def buf(max_size=5, Tb=6, B=3, **kw):
    return PrioritizedReplayBuffer(max_size=max_size, sample_length=Tb, batch_size=B, warmup_transitions=kw.pop("warmup", 0), **kw)


# ------------------------------------------------------------------------------------------------ the reference's trees
@pytest.mark.parametrize("capacity", [8, 64])
def test_every_tree_node_after_every_assignment(g, capacity):
    key = f"tree{capacity}"
    st, mt = np.zeros(2 * capacity), np.full(2 * capacity, np.inf)
    for k, (s, v) in enumerate(zip(g[key + "_slots"], g[key + "_leaves"])):
        replay.set_leaves(st, mt, [s], [v])
        assert np.array_equal(st, g[key + "_sum"][k]) and np.array_equal(mt, g[key + "_min"][k]), k
    # ... and all in one call: a repeated slot keeps its last value
    st2, mt2 = np.zeros(2 * capacity), np.full(2 * capacity, np.inf)
    replay.set_leaves(st2, mt2, g[key + "_slots"], g[key + "_leaves"])
    assert np.array_equal(st2, st) and np.array_equal(mt2, mt)


@pytest.mark.parametrize("capacity", [8, 64])
def test_find_prefixsum_idx_on_and_off_the_boundaries(g, capacity):
    key = f"tree{capacity}"
    st = g[key + "_sum"][-1]
    masses, found = g[key + "_masses"], g[key + "_found"]
    bounds = np.cumsum(st[capacity:])
    assert np.isin(bounds, masses).all() and st[1] in masses  # the fixture does hold every boundary and the root
    assert np.array_equal(replay.find_prefixsum_idx(st, masses), found)
    assert np.array_equal([int(replay.find_prefixsum_idx(st, m)) for m in masses[:16]], found[:16])  # scalar masses too


def test_non_integer_leaves(g):
    st, mt = np.zeros(16), np.full(16, np.inf)
    replay.set_leaves(st, mt, np.arange(8), g["pow_leaves"])
    assert np.array_equal(st, g["pow_sum"]) and np.array_equal(mt, g["pow_min"])
    # difference (b): the leaf is float64 pow of the float32 priority (numpy's pow here and the generator's may differ in the last bit)
    mine = replay.leaf_values(g["pow_priorities"], 0.6)
    assert mine.dtype == np.float64 and np.allclose(mine, g["pow_leaves"], rtol=4 * np.finfo(np.float64).eps, atol=0)
    p = g["pow_priorities"]
    assert np.array_equal(replay.leaf_values(p, 1.0), p.astype(np.float64)) and (replay.leaf_values(p, 0.0) == 1.0).all()


# ------------------------------------------------------------------------------------------------ the reference's buffer
def test_initial_priorities(g):
    b = buf(burn_in_steps=1, alpha=1.0, priority_interpolation_eta=0.9)
    for k in range(5):
        b.put(make_sample(6, k, ret=g["init_ret"][k], value=g["init_value"][k]))
    got = b.sum_tree[b.capacity:b.capacity + 5].astype(np.float32)
    assert (ulp32(got, g["init_priorities"]) <= 1).all(), (got, g["init_priorities"])
    # no analyzed_result.ret: the running max_priority
    c = buf(alpha=1.0, max_priority=1.0)
    c.put(make_sample(6, 0))
    assert c.sum_tree[c.capacity] == float(g["init_default"][0]) == 1.0
    with pytest.raises(ValueError):  # ret without an eta
        buf().put(make_sample(6, 0, ret=g["init_ret"][0], value=g["init_value"][0]))


def test_update_rounds_trees_max_priority_beta_and_weights(g):
    b = buf(burn_in_steps=1, alpha=1.0, beta=0.4, beta_scheduler=LinearScheduler(0.4, 10, 1.0), max_priority=1.0,
            priority_interpolation_eta=0.9)
    for k in range(5):
        b.put(make_sample(6, k))
    # the leaves the generator filled the reference's trees with
    b._set(np.arange(5), g["init_priorities"], 5)
    b._max_priority = np.float32(1.0)
    for r in range(g["upd_idxes"].shape[0]):
        idx = g["upd_idxes"][r]
        cap, total, filled = b.capacity, b.sum_tree[1], np.float64(5)
        w = (np.power(b.sum_tree[cap + idx] / total * filled, -np.float64(b.beta)) /
             np.power(b.min_tree[1] / total * filled, -np.float64(b.beta))).astype(np.float32)
        assert (ulp32(w, g["upd_weights"][r]) <= 1).all(), (r, w, g["upd_weights"][r])
        b.update_priorities(idx, g["upd_priorities"][r])
        assert np.array_equal(b.sum_tree, g["upd_sum"][r]) and np.array_equal(b.min_tree, g["upd_min"][r]), r
        assert np.float32(b.max_priority) == g["upd_max_priority"][r], r
        assert b.beta == g["upd_beta"][r], (r, b.beta, g["upd_beta"][r])
    assert g["upd_max_priority"][-1] > 1.0 and g["upd_beta"][-1] > 0.4  # the fixture did move both


def test_get_weights_are_the_statement_of_the_recorded_ones(g):
    """``get`` hands out, for the indices it drew, the weights the reference's expressions give over the same trees."""
    b = buf(alpha=1.0, beta=0.4)
    for k in range(5):
        b.put(make_sample(6, k))
    b._set(np.arange(5), g["init_priorities"], 5)
    e = b.get()
    idx, w = e.sampling_indices, e.sample.metadata["sampling_weight"]
    assert idx.dtype == np.int32 and w.dtype == np.float32 and (np.diff(idx) >= 0).all()
    total, mn = float(b.sum_tree[1]), float(b.min_tree[1])
    want = [(float(b.sum_tree[b.capacity + i]) / total * 5)**(-0.4) / (mn / total * 5)**(-0.4) for i in idx]
    assert (ulp32(w, np.array(want, np.float32)) <= 1).all()


# ------------------------------------------------------------------------------------------------ the differences
def test_the_newest_slot_is_drawn():
    """Difference (a): the total mass is the root.  With k equal priorities and k draws, stratum i lies in slot i: every filled
    slot is drawn, the newest included (the reference's total leaves it out)."""
    for k in (1, 2, 5):
        b = buf(max_size=8, B=k, alpha=0.6)
        for j in range(k):
            b.put(make_sample(6, j))
        assert np.array_equal(b.get().sampling_indices, np.arange(k)), k
    # ... and a mass equal to the root is clamped to the last filled slot, not walked into an empty leaf
    b = buf(max_size=8, B=3, alpha=1.0)
    for j in range(5):
        b.put(make_sample(6, j))
    assert replay.find_prefixsum_idx(b.sum_tree, b.sum_tree[1]) >= 5
    assert min(replay.find_prefixsum_idx(b.sum_tree, b.sum_tree[1]), 5 - 1) == 4


def test_draws_follow_the_philox_counter_layout():
    """Difference (c): the restatement of tests/loss_ref.py, word by word."""
    import loss_ref
    seed, offset, n = 0x123456789ABCDEF, 7, 70
    r = np.arange(n, dtype=np.uint64)
    m32 = np.uint64(0xFFFFFFFF)
    ctr = np.stack([r & m32, r >> np.uint64(32), np.zeros(n, np.uint64), np.full(n, offset, np.uint64)], -1)
    x = loss_ref.philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64))[:, 0]
    u = replay.stratified_uniforms(n, seed, offset)
    assert np.array_equal(u, (x >> np.uint64(8)).astype(np.float64) * 2.0**-24) and (u >= 0).all() and (u < 1).all()
    # successive gets take successive offsets
    b = buf(max_size=64, B=8, seed=3)
    for j in range(64):
        b.put(make_sample(6, j))
    first, second = b.get().sampling_indices, b.get().sampling_indices
    want = [replay.sample_proportional(b.sum_tree, b.min_tree, 64, 8, 0.4, 3, o)[0] for o in (0, 1)]
    assert np.array_equal(first, want[0]) and np.array_equal(second, want[1]) and not np.array_equal(first, second)


def test_refused_priorities_raise_and_change_nothing():
    b = buf(alpha=1.0)
    for j in range(5):
        b.put(make_sample(6, j))
    before = (b.sum_tree.copy(), b.min_tree.copy(), b.max_priority, b.beta)
    for bad in (np.nan, np.inf, 0.0, -1.0):
        with pytest.raises(ValueError):
            b.update_priorities(np.array([0, 1, 2]), np.array([2.0, bad, 3.0], np.float32))
    with pytest.raises(ValueError):
        b.update_priorities(np.array([0, 1, 5]), np.array([2.0, 1.0, 3.0], np.float32))  # slot 5 is not filled
    with pytest.raises(ValueError):
        b.update_priorities(np.array([0, 1]), np.array([2.0, 1.0], np.float32))  # not batch_size pairs
    assert np.array_equal(b.sum_tree, before[0]) and np.array_equal(b.min_tree, before[1])
    assert (b.max_priority, b.beta) == before[2:]


# ------------------------------------------------------------------------------------------------ the interface
def test_constructor_validation():
    with pytest.raises(ValueError, match="alpha"):
        buf(alpha=-0.1)
    with pytest.raises(ValueError, match="beta"):
        buf(beta=0.0)
    with pytest.raises(ValueError, match="init_value"):
        buf(beta=0.4, beta_scheduler=LinearScheduler(0.5, 10, 1.0))
    b = buf(alpha=0.0, beta_scheduler=types.SimpleNamespace(init_value=0.4, get=lambda step: 0.4 + step))  # any object with get(step)
    assert b.capacity == 8 and b.beta == 0.4
    assert buf(max_size=1).capacity == 1 and buf(max_size=2).capacity == 2 and buf(max_size=2048).capacity == 2048
    with pytest.raises(RuntimeError, match="sample length"):
        b.put(make_sample(5, 0))


def test_counters_and_wrap_around():
    b = buf(max_size=5, Tb=6, B=3, warmup=12, alpha=1.0)
    assert b.empty() and not b.full() and b.qsize() == 0
    for j in range(5):
        b.put(make_sample(6, j))
        assert b.qsize() == 6 * (j + 1) and b.empty() == (j < 1)
    assert b.full()
    b.update_priorities(np.array([0, 1, 2]), np.array([7.0, 0.5, 0.25], np.float32))
    assert b.max_priority == 7.0
    b.put(make_sample(6, 9))  # overwrites the oldest slot, 0, with the running max_priority
    assert b.full() and b.qsize() == 30 and b.sum_tree[b.capacity] == 7.0
    b.put(make_sample(6, 10))  # slot 1
    # batch_size draws over five slots; every leaf of the batch is [Tb, B, ...] and row b is slot idx[b]'s sample
    e = b.get()
    idx, s = e.sampling_indices, e.sample
    assert s.obs.obs.shape == (6, 3, 3, 4) and s.obs.obs.dtype == np.uint8 and s.reward.shape == (6, 3, 1)
    owner = {0: 9, 1: 10, 2: 2, 3: 3, 4: 4}
    for col, slot in enumerate(idx):
        want = make_sample(6, owner[int(slot)])
        assert np.array_equal(s.obs.obs[:, col], want.obs.obs) and np.array_equal(s.reward[:, col], want.reward)
        assert np.array_equal(s.on_reset[:, col], want.on_reset)
    assert e.reuses_left == -1 and e.receive_time == -1 and s.analyzed_result is None


def test_make_buffer_names():
    b = buffer_mod.make_buffer("prioritized_replay_buffer", max_size=4, sample_length=3, batch_size=2, warmup_transitions=0)
    assert isinstance(b, PrioritizedReplayBuffer)
    assert isinstance(buffer_mod.make_buffer("priority_queue", max_size=4), buffer_mod.PriorityQueueBuffer)
    for name in ("simple_queue", "simple_replay_buffer"):
        with pytest.raises(NotImplementedError):
            buffer_mod.make_buffer(name)
    with pytest.raises(KeyError):
        buffer_mod.make_buffer("no_such_buffer")
    import torch
    from srl_amd import hip
    if not torch.cuda.is_available():  # the device buffer fails loudly without a GPU
        with pytest.raises(hip.HipError):
            buffer_mod.make_buffer("prioritized_replay_buffer_hip", max_size=4, sample_length=3, batch_size=2, warmup_transitions=0)
    assert buffer_mod.ReplayEntry(1, 0.0, None).sampling_indices is None
