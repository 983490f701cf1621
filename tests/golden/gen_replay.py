"""Generate tests/golden/replay.npz: the REAL reference's segment trees and the bookkeeping of its PrioritizedReplayBuffer (read-only
beside this repository), on the CPU.

Run (from the repo root):
    CUDA_VISIBLE_DEVICES="" PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout> python3 tests/golden/gen_replay.py

Harness-side shims (the reference files stay untouched): a numpy alias and MagicMock for import-time dependencies that are absent.

What it records:
  * ``tree<c>_*`` for capacities 8 and 64: a sequence of (slot, leaf) assignments with repeated slots, driven through
    ``SumSegmentTree`` / ``MinSegmentTree.__setitem__``; every node of both trees after every assignment; then masses -- every
    prefix sum of the (integer-valued, so exact) leaves, i.e. each leaf boundary, the root itself, 0, and random ones -- with the
    ``find_prefixsum_idx`` of each;
  * ``pow_*``: capacity 8 with leaves ``float64(p) ** 0.6``, final nodes only (the test assigns the recorded leaves);
  * ``init_*``: ``PrioritizedReplayBuffer._compute_init_priorities`` on samples with ``analyzed_result.ret / value`` (burn_in_steps 1,
    eta 0.9) and on one without;
  * ``upd_*``: ``update_priorities`` rounds on a buffer of max_size 5 (alpha 1, a linear beta schedule 0.4 -> 1.0 over 10 steps)
    whose trees were filled with recorded priorities, the new priorities handed over as float64 copies of float32 values: both
    trees, ``_max_priority`` and ``_beta`` after every round, and the importance weights of recorded indices by the reference's
    expressions (buffer.py:430-437) over its trees.
"""
import os
import sys
import types

import numpy as np

np.bool8 = np.bool_
from unittest import mock

for m in ["gym", "gym.spaces", "redis", "redis.backoff", "redis.retry", "wandb", "zmq", "blosc"]:
    sys.modules.setdefault(m, mock.MagicMock())
sys.modules.setdefault("mock", mock)

import base.timeutil
from base.buffer import PrioritizedReplayBuffer
from base.segment_tree import MinSegmentTree, SumSegmentTree

HERE = os.path.dirname(os.path.abspath(__file__))


def drive_trees(out, key, capacity, slots, leaves, rng, n_random):
    st, mt = SumSegmentTree(capacity), MinSegmentTree(capacity)
    snaps_s, snaps_m = [], []
    for s, v in zip(slots, leaves):
        st[int(s)] = float(v)
        mt[int(s)] = float(v)
        snaps_s.append(np.array(st._value, np.float64))
        snaps_m.append(np.array(mt._value, np.float64))
    out[key + "_slots"], out[key + "_leaves"] = np.asarray(slots, np.int64), np.asarray(leaves, np.float64)
    out[key + "_sum"], out[key + "_min"] = np.stack(snaps_s), np.stack(snaps_m)
    final = np.array(st._value[capacity:], np.float64)
    bounds = np.concatenate([[0.0], np.cumsum(final)])  # exact: integer-valued leaves
    masses = np.concatenate([bounds, np.nextafter(bounds[1:], 0.0), np.nextafter(bounds[:-1], np.inf),
                             rng.random(n_random) * st.sum()])
    assert (masses >= 0).all() and (masses <= st.sum() + 1e-5).all()
    out[key + "_masses"] = masses
    out[key + "_found"] = np.array([st.find_prefixsum_idx(float(m)) for m in masses], np.int64)
    return st, mt


def main():
    rng = np.random.default_rng(20260)
    out = {}
    # ---- trees: integer-valued leaves (exact sums: a mass can sit exactly on a boundary), repeated slots, an empty tail
    for capacity, n_slots, n_ops in ((8, 5, 12), (64, 50, 150)):
        slots = np.concatenate([np.arange(n_slots), rng.integers(0, n_slots, size=n_ops)])
        leaves = rng.integers(1, 9, size=slots.size).astype(np.float64)
        drive_trees(out, f"tree{capacity}", capacity, slots, leaves, rng, 64)
    # ---- non-integer leaves: float64(p) ** 0.6
    p = (rng.random(8) * 4 + 0.01).astype(np.float32)
    leaves = np.power(p.astype(np.float64), 0.6)
    st, mt = SumSegmentTree(8), MinSegmentTree(8)
    for s, v in enumerate(leaves):
        st[s] = float(v)
        mt[s] = float(v)
    out["pow_priorities"], out["pow_leaves"] = p, leaves
    out["pow_sum"], out["pow_min"] = np.array(st._value, np.float64), np.array(mt._value, np.float64)

    # ---- the buffer's bookkeeping
    Tb, max_size, B = 6, 5, 3
    sched = base.timeutil.LinearScheduler(init_value=0.4, total_iters=10, end_value=1.0)
    buf = PrioritizedReplayBuffer(max_size=max_size, sample_length=Tb, batch_size=B, warmup_transitions=0, seed=0, burn_in_steps=1,
                                  alpha=1.0, beta=0.4, beta_scheduler=sched, max_priority=1.0, priority_interpolation_eta=0.9)
    ret = rng.normal(size=(max_size, Tb, 1)).astype(np.float32)
    value = rng.normal(size=(max_size, Tb, 1)).astype(np.float32)
    init = []
    for k in range(max_size):
        sample = types.SimpleNamespace(analyzed_result=types.SimpleNamespace(ret=ret[k], value=value[k]))
        init.append(np.asarray(buf._compute_init_priorities(sample), np.float32).reshape(1))
    out["init_ret"], out["init_value"], out["init_priorities"] = ret, value, np.concatenate(init)
    none = types.SimpleNamespace(analyzed_result=types.SimpleNamespace(ret=None, value=None))
    out["init_default"] = np.asarray(buf._compute_init_priorities(none), np.float32).reshape(1)
    # fill the trees as put does (buffer.py:391-393, alpha = 1: the leaf is the priority), without its pinned host store
    for k in range(max_size):
        buf._sum_tree[k] = float(out["init_priorities"][k])
        buf._min_tree[k] = float(out["init_priorities"][k])
    buf._total_chunks = max_size
    buf._total_transitions = max_size * Tb
    rounds = 6
    idxes = np.sort(rng.integers(0, max_size, size=(rounds, B)), axis=1)
    idxes[2] = [1, 1, 4]  # a repeated slot: the last one stands
    pri = (rng.random((rounds, B)) * 3 + 0.05).astype(np.float32)
    sums, mins, maxp, betas, weights = [], [], [], [], []
    for r in range(rounds):
        # the weights get() would hand out for these indices, by its expressions over the reference's trees (:430-437)
        p_min = buf._min_tree.min() / buf._sum_tree.sum()
        max_weight = (p_min * buf._total_chunks)**(-buf._beta)
        weights.append(np.array([(buf._sum_tree[int(i)] / buf._sum_tree.sum() * buf._total_chunks)**(-buf._beta) / max_weight
                                 for i in idxes[r]], dtype=np.float32))
        # float64 copies of the float32 priorities: the reference's leaf is `priority ** alpha` in the priority's own precision,
        # and a float32 leaf would make its inner nodes float32 sums (this repository's difference (b))
        buf.update_priorities(idxes[r], pri[r].astype(np.float64))
        sums.append(np.array(buf._sum_tree._value, np.float64))
        mins.append(np.array(buf._min_tree._value, np.float64))
        maxp.append(np.float32(buf._max_priority))
        betas.append(np.float64(buf._beta))
    out["upd_idxes"], out["upd_priorities"] = idxes.astype(np.int64), pri
    out["upd_sum"], out["upd_min"] = np.stack(sums), np.stack(mins)
    out["upd_max_priority"], out["upd_beta"], out["upd_weights"] = np.array(maxp, np.float32), np.array(betas), np.stack(weights)
    path = os.path.join(HERE, "replay.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
