"""Prioritised experience replay for the Q-learning family: a host statement in numpy and a buffer resident in HBM.

Counterpart of the reference's ``PrioritizedReplayBuffer`` (``base/buffer.py:280-465``) over its two segment trees
(``base/segment_tree.py``): the same constructor keywords, defaults and validation errors, ``put`` of one ``[Tb, ...]`` sample into
slot ``ptr`` with an initial priority from ``analyzed_result.ret / value`` or ``max_priority`` (``:350-361``), ``get`` of
``batch_size`` stratified draws proportional to ``priority ** alpha`` with importance weights in ``sampling_weight`` and the drawn
slots in ``ReplayEntry.sampling_indices`` (``:409-447``), ``update_priorities`` with the trainer's new priorities (``:449-462``).

``PrioritizedReplayBuffer`` is plain numpy and needs no GPU.  It is the float64 statement of the kernels in ``csrc/replay.hip`` and
the reference the device tests hold them to.  ``DevicePrioritizedReplayBuffer`` keeps the store, both trees, ``max_priority`` and
the priorities in HBM: ``get`` draws (``srl_per_sample``), gathers every leaf time-major (``srl_replay_gather``) and returns device
tensors without waiting for the device; ``update_priorities`` takes the device tensor ``DeepQLearning.step(...,
device_priorities=True)`` returns (``srl_per_set``).  A replayed frame crosses the host link once, when it is put.

DIFFERENCES from the reference, in both buffers:
  (a) the total mass of a draw is the ROOT of the sum tree.  The reference takes ``sum(0, total_chunks - 1)`` (``:411``), a half-open
      range that leaves the newest filled slot out, so that slot is never drawn (over leaves 1..5, ``sum(0, 4)`` is 10 and the root
      15).  A mass that rounds up to the root is clamped to the last filled slot.
  (b) a leaf is the float64 ``pow`` of the float32 priority; the reference's precision depends on the numpy version.
  (c) the uniform draws come from Philox4x32-10 with the samplers' counter layout (row = the draw's number, stream word 0, offset =
      the number of ``get`` calls before this one, key = ``seed``), not from Python's ``random``.
  (d) a priority that is not finite or not > 0, or a slot that is not filled, is refused: ``PrioritizedReplayBuffer`` raises
      ``ValueError`` before it changes anything (the reference asserts part-way through its loop), the device buffer leaves the leaf
      alone and counts it (``refused_count()``) -- it cannot raise without a host wait, and the TD kernel gives NaN for a column whose
      loss rows are all done.
  (e) the device buffer keeps no replay-time log: ``ReplayEntry.reuses`` is 0 there.
"""
import math

import numpy as np

from srl_amd.namedarray import flatten, from_flattened
from srl_amd.runtime.buffer import ReplayEntry


class ConstantScheduler:
    """``base/timeutil.py:130-133``."""

    def __init__(self, init_value, total_iters=math.inf):
        self.init_value, self.total_iters = init_value, total_iters

    def get(self, step):
        return self.init_value


class LinearScheduler:
    """``base/timeutil.py:137-141``, with its range check (``:114-119``)."""

    def __init__(self, init_value, total_iters, end_value):
        if total_iters <= 0:
            raise ValueError("total_iters should be a positive number.")
        self.init_value, self.total_iters, self.end_value = init_value, total_iters, end_value

    def get(self, step):
        if step < 0 or step > self.total_iters:
            raise ValueError(f"Scheduler step should be in the interval [0, {self.total_iters}]. Input {step}.")
        return (self.end_value - self.init_value) / self.total_iters * step + self.init_value


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al. 2011) on uint64 arrays of 32-bit words: counter [..., 4], key [2] -> the four output words
    [..., 4].  The statement of ``csrc/action_dist.h``."""
    m32, sh = np.uint64(0xFFFFFFFF), np.uint64(32)
    M0, M1, W0, W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    c = [np.asarray(counter, np.uint64)[..., i] & m32 for i in range(4)]
    k = [np.uint64(key[0]) & m32, np.uint64(key[1]) & m32]
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> sh) ^ c[1] ^ k[0], p1 & m32, (p0 >> sh) ^ c[3] ^ k[1], p0 & m32]
        k = [(k[0] + W0) & m32, (k[1] + W1) & m32]
    return np.stack(c, -1)


def stratified_uniforms(n, seed, offset):
    """u[i] = (x0 >> 8) 2^-24 of the draw with counter {i, 0, 0, offset low word} and key {seed low, seed high}: float64, exact."""
    m32 = np.uint64(0xFFFFFFFF)
    i = np.arange(n, dtype=np.uint64)
    seed, offset = np.uint64(int(seed) & (2**64 - 1)), np.uint64(int(offset) & (2**64 - 1))
    ctr = np.stack([i & m32, i >> np.uint64(32), np.zeros(n, np.uint64), np.broadcast_to(offset & m32, i.shape)], -1)
    x0 = philox4x32_10(ctr, (seed & m32, seed >> np.uint64(32)))[:, 0]
    return (x0 >> np.uint64(8)).astype(np.float64) * 2.0**-24


def tree_capacity(max_size):
    capacity = 1
    while capacity < max_size:
        capacity *= 2
    return capacity


def leaf_values(priorities, alpha):
    """``pow((double)priority, alpha)`` of float32 priorities; alpha 1 and 0 give the priority and 1.0 exactly."""
    x = np.asarray(priorities, np.float32).astype(np.float64)
    if alpha == 1.0:
        return x
    if alpha == 0.0:
        return np.ones_like(x)
    return np.power(x, np.float64(alpha))


def set_leaves(sum_tree, min_tree, slots, leaves):
    """``SegmentTree.__setitem__`` (``segment_tree.py:75-82``) on both trees, pair by pair: a repeated slot keeps its last value."""
    capacity = sum_tree.size // 2
    for s, v in zip(slots, leaves):
        node = capacity + int(s)
        sum_tree[node] = min_tree[node] = v
        node //= 2
        while node >= 1:
            sum_tree[node] = sum_tree[2 * node] + sum_tree[2 * node + 1]
            a, b = min_tree[2 * node], min_tree[2 * node + 1]
            min_tree[node] = b if b < a else a  # Python's min(a, b)
            node //= 2


def find_prefixsum_idx(sum_tree, mass):
    """``find_prefixsum_idx`` (``segment_tree.py:117-124``) for a vector of masses: left iff value[2 node] > mass, else subtract and
    go right.  Every draw walks the same number of levels."""
    capacity = sum_tree.size // 2
    mass = np.array(mass, np.float64)
    node = np.ones(mass.shape, np.int64)
    level = 1
    while level < capacity:
        left = sum_tree[2 * node]
        go_left = left > mass
        mass = np.where(go_left, mass, mass - left)
        node = np.where(go_left, 2 * node, 2 * node + 1)
        level *= 2
    return node - capacity


def sample_proportional(sum_tree, min_tree, n_filled, batch_size, beta, seed, offset):
    """The float64 statement of ``srl_per_sample``: (idx int32 [B] ascending, weight float32 [B], mass float64 [B])."""
    capacity = sum_tree.size // 2
    total = sum_tree[1]
    u = stratified_uniforms(batch_size, seed, offset)
    mass = (u + np.arange(batch_size, dtype=np.float64)) * (total / np.float64(batch_size))
    idx = np.minimum(find_prefixsum_idx(sum_tree, mass), n_filled - 1)
    filled = np.float64(n_filled)
    w = np.power(sum_tree[capacity + idx] / total * filled, -np.float64(beta))
    w_max = np.power(min_tree[1] / total * filled, -np.float64(beta))
    return idx.astype(np.int32), (w / w_max).astype(np.float32), mass


class _PrioritizedReplayBase:
    """Constructor, counters, the initial priority and the beta schedule: what the two buffers share."""

    def __init__(self, max_size, sample_length, batch_size, warmup_transitions, seed=0, burn_in_steps=0, alpha=0.6, beta=0.4,
                 beta_scheduler=None, max_priority=1.0, priority_interpolation_eta=None):
        if alpha < 0:
            raise ValueError("`alpha` must be a non-negative number.")
        if beta <= 0:
            raise ValueError("`beta` must be a positive number.")
        if beta_scheduler is None:
            beta_scheduler = ConstantScheduler(init_value=beta, total_iters=math.inf)
        if beta_scheduler.init_value != beta:
            raise ValueError("`init_value` of `beta_scheduler` should be the same as the `beta` argument.")
        if max_size < 1 or batch_size < 1 or sample_length < 1:
            raise ValueError("`max_size`, `batch_size` and `sample_length` must be positive.")
        if not (math.isfinite(max_priority) and max_priority > 0):
            raise ValueError("`max_priority` must be a positive number.")
        self._max_size, self._sample_length, self._batch_size = int(max_size), int(sample_length), int(batch_size)
        self._warmup_transitions = warmup_transitions
        self._seed, self._burn_in_steps = int(seed), int(burn_in_steps)
        self._alpha, self._beta, self._beta_scheduler = float(alpha), beta, beta_scheduler
        self._eta, self._init_max_priority = priority_interpolation_eta, max_priority
        self._capacity = tree_capacity(self._max_size)
        self._total_transitions = self._total_chunks = self._ptr = 0
        self._training_steps = self._gets = 0
        self._keys = None

    # the reference's n_chunks_per_sample is 1 here (it asserts so for this buffer, :329)
    def qsize(self):
        return self._total_transitions

    def empty(self):
        return self._total_transitions < self._warmup_transitions

    def full(self):
        return self._total_transitions == self._max_size * self._sample_length

    @property
    def beta(self):
        return self._beta

    @property
    def capacity(self):
        return self._capacity

    def _init_priority(self, sample):
        """``_compute_init_priorities`` (``:350-361``) in the reference's float32; None: take the running ``max_priority``."""
        ar = getattr(sample, "analyzed_result", None)
        ret = getattr(ar, "ret", None) if ar is not None else None
        if ret is None:
            return None
        if self._eta is None:
            raise ValueError("`priority_interpolation_eta` is needed for samples that carry `analyzed_result.ret`.")
        td_err = np.abs(np.asarray(ret) - np.asarray(ar.value)).squeeze(-1)[self._burn_in_steps:]
        priority = self._eta * td_err.max(keepdims=True) + (1 - self._eta) * td_err.mean(keepdims=True)
        if priority.shape != (1,):
            raise ValueError(f"one priority per sample expected, got shape {priority.shape}")
        return priority.astype(np.float32)

    def _leaves_of(self, x):
        if hasattr(x, "policy_name"):
            x.policy_name = None  # as the reference does (:365-367)
        if x.length(0) != self._sample_length:
            raise RuntimeError("The sample received in PrioritizedReplayBuffer has a different sample length from configuration! "
                               f"({x.length(0)} vs {self._sample_length})")
        return [(k, None if v is None else np.asarray(v)) for k, v in flatten(x)]

    def _advance(self):
        self._total_transitions = min(self._total_transitions + self._sample_length, self._max_size * self._sample_length)
        self._total_chunks = min(self._max_size, self._total_chunks + 1)
        self._ptr = (self._ptr + 1) % self._max_size

    def _check_update(self, idxes, priorities):
        if tuple(idxes.shape) != (self._batch_size,) or tuple(priorities.shape) != (self._batch_size,):
            raise ValueError(f"expected {self._batch_size} indices and priorities, got {tuple(idxes.shape)} and {tuple(priorities.shape)}")

    def _updated(self):
        self._training_steps += 1
        self._beta = self._beta_scheduler.get(self._training_steps)


class PrioritizedReplayBuffer(_PrioritizedReplayBase):
    """The host buffer: numpy stores ``[max_size, Tb, ...]``, float64 trees, every step the statement of a kernel."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.sum_tree = np.zeros(2 * self._capacity, np.float64)
        self.min_tree = np.full(2 * self._capacity, np.inf, np.float64)
        self._max_priority = np.float32(self._init_max_priority)
        self._replay_times = np.zeros(self._max_size, np.int64)
        self._store = None

    @property
    def max_priority(self):
        return float(self._max_priority)

    def put(self, x):
        leaves = self._leaves_of(x)
        if self._store is None:
            self._keys = [k for k, _ in leaves]
            self._store = [None if v is None else np.zeros((self._max_size, *v.shape), v.dtype) for _, v in leaves]
        for store, (_, v) in zip(self._store, leaves):
            if store is not None:
                store[self._ptr] = v
        priority = self._init_priority(x)
        self._set(np.array([self._ptr]), np.array([self._max_priority]) if priority is None else priority, self._ptr + 1)
        self._replay_times[self._ptr] = 0
        self._advance()

    def _set(self, slots, priorities, n_slots):
        slots, priorities = np.asarray(slots), np.asarray(priorities, np.float32)
        bad = ~(np.isfinite(priorities) & (priorities > 0))
        if bad.any():
            raise ValueError(f"priorities must be finite and > 0, got {priorities[bad][:8]}")
        if ((slots < 0) | (slots >= n_slots)).any():
            raise ValueError(f"slots must lie in [0, {n_slots}), got {slots[(slots < 0) | (slots >= n_slots)][:8]}")
        set_leaves(self.sum_tree, self.min_tree, slots, leaf_values(priorities, self._alpha))
        self._max_priority = max(self._max_priority, priorities.max())

    def get(self):
        assert self._total_chunks > 0, "attempting to get from empty buffer."
        idx, weight, _ = sample_proportional(self.sum_tree, self.min_tree, self._total_chunks, self._batch_size, self._beta, self._seed,
                                             self._gets)
        assert (np.diff(idx) >= 0).all(), "stratified draws come out ascending"
        self._gets += 1
        data = from_flattened([(k, None if s is None else np.ascontiguousarray(np.swapaxes(s[idx], 0, 1)))
                               for k, s in zip(self._keys, self._store)])
        data.register_metadata(sampling_weight=weight)
        return ReplayEntry(reuses_left=-1, receive_time=-1, sample=data, reuses=self._replay_times[idx].mean(), sampling_indices=idx)

    def update_priorities(self, idxes, priorities):
        idxes, priorities = np.asarray(idxes), np.asarray(priorities)
        self._check_update(idxes, priorities)
        self._set(idxes, priorities, self._total_chunks)
        np.add.at(self._replay_times, idxes, 1)
        self._updated()


class DevicePrioritizedReplayBuffer(_PrioritizedReplayBase):
    """The same buffer with the store ``[max_size, Tb, row]`` per leaf, both trees and ``max_priority`` in HBM.  A leaf keeps its
    dtype; a row that is no multiple of 4 bytes (a flag per step) is padded to one in the store and in the gathered batch, and
    comes back at its own width (a device copy of that narrow leaf)."""

    def __init__(self, *args, device="cuda", **kwargs):
        super().__init__(*args, **kwargs)
        import torch
        from srl_amd import hip
        hip.require_gpu()
        self._torch, self._hip = torch, hip
        self.device = torch.device(device)
        cap = self._capacity
        self.sum_tree = torch.zeros(2 * cap, dtype=torch.float64, device=self.device)
        self.min_tree = torch.full((2 * cap,), math.inf, dtype=torch.float64, device=self.device)
        self._last = torch.full((cap,), -1, dtype=torch.int32, device=self.device)
        # the state block: max_priority (float32) and the count of refused priorities (int32)
        self._state = torch.zeros(2, dtype=torch.int32, device=self.device)
        self._max_priority, self._refused = self._state[:1].view(torch.float32), self._state[1:]
        self._max_priority.fill_(float(np.float32(self._init_max_priority)))
        self._store = None

    # ---- host reads of the device state: each waits for the device
    @property
    def max_priority(self):
        return float(self._max_priority.item())

    def refused_count(self):
        return int(self._refused.item())

    def put(self, x):
        torch = self._torch
        leaves = self._leaves_of(x)
        if self._store is None:
            self._keys, self._store = [k for k, _ in leaves], []
            for _, v in leaves:
                if v is None:
                    self._store.append(None)
                    continue
                v = v.view(np.uint8) if v.dtype == np.bool_ else v
                row = int(np.prod(v.shape[1:], dtype=np.int64)) * v.dtype.itemsize
                pad = -(-row // 4) * 4
                self._store.append(dict(bytes=torch.zeros((self._max_size, self._sample_length, pad), dtype=torch.uint8, device=self.device),
                                        row=row, pad=pad, shape=tuple(v.shape[1:]), dtype=torch.from_numpy(v[:0]).dtype))
        for s, (_, v) in zip(self._store, leaves):
            if s is None:
                continue
            host = torch.from_numpy(np.ascontiguousarray(v).view(np.uint8).reshape(self._sample_length, s["row"]))
            s["bytes"][self._ptr, :, :s["row"]].copy_(host, non_blocking=True)
        priority = self._init_priority(x)
        slot = torch.tensor([self._ptr], dtype=torch.int32).to(self.device, non_blocking=True)
        # without analyzed_result.ret the running max_priority is the priority: read where it lives, on the device
        pri = self._max_priority if priority is None else torch.from_numpy(priority).to(self.device, non_blocking=True)
        self._set(slot, pri, self._ptr + 1)
        self._advance()

    def _set(self, slots, priorities, n_slots):
        self._hip.per_set(self.sum_tree, self.min_tree, self._capacity, n_slots, slots, priorities, self._alpha, self._last,
                          self._max_priority, self._refused)

    def get(self):
        torch, hip = self._torch, self._hip
        assert self._total_chunks > 0, "attempting to get from empty buffer."
        B, Tb = self._batch_size, self._sample_length
        idx = torch.empty(B, dtype=torch.int32, device=self.device)
        weight = torch.empty(B, dtype=torch.float32, device=self.device)
        hip.per_sample(self.sum_tree, self.min_tree, self._capacity, self._total_chunks, self._beta, self._seed, self._gets, idx, weight)
        self._gets += 1
        entries = []
        for k, s in zip(self._keys, self._store):
            if s is None:
                entries.append((k, None))
                continue
            out = torch.empty((Tb, B, s["pad"]), dtype=torch.uint8, device=self.device)
            hip.replay_gather(s["bytes"].data_ptr(), self._max_size, idx, B, Tb, s["pad"], out.data_ptr())
            leaf = out if s["pad"] == s["row"] else out[:, :, :s["row"]].contiguous()  # (a device copy of a narrow leaf)
            entries.append((k, leaf.view(s["dtype"]).view(Tb, B, *s["shape"])))
        data = from_flattened(entries)
        data.register_metadata(sampling_weight=weight)
        return ReplayEntry(reuses_left=-1, receive_time=-1, sample=data, reuses=0, sampling_indices=idx)

    def update_priorities(self, idxes, priorities):
        torch = self._torch
        if not isinstance(idxes, torch.Tensor):
            idxes = torch.from_numpy(np.ascontiguousarray(idxes, dtype=np.int32))
        if not isinstance(priorities, torch.Tensor):
            priorities = torch.from_numpy(np.ascontiguousarray(priorities, dtype=np.float32))
        self._check_update(idxes, priorities)
        idxes = idxes.to(device=self.device, dtype=torch.int32, non_blocking=True).contiguous()
        priorities = priorities.to(device=self.device, dtype=torch.float32, non_blocking=True).contiguous()
        self._set(idxes, priorities, self._total_chunks)
        self._updated()
