"""The prioritised-replay kernels (csrc/replay.hip) through srl_amd/hip.py against the host buffer's float64 statement
(srl_amd/runtime/replay.py), at the smallest shapes that can go wrong: capacities 1, 2, 8 (max_size 5), 2048 and 131072; 1, 3, 64,
65, 300 and 1500 pairs / draws at capacity 2048 (one wavefront and one past it, more than the set kernel's 1024 threads), and 300 at
max_size 5 (more pairs than slots: forced duplicates).

Bounds.  alpha 1 and 0: every node of both trees bit-exact.  alpha 0.6: a leaf within 16 float64 ulp of numpy's pow -- the bound
OpenCL's specification puts on double pow, which the device library is built to -- and every inner node the exact sum / min of the
device's OWN two children.  Draws: the host descent runs on the device's own tree and must give the same indices; weights within
1 float32 ulp (the float64 error of either side is far below half a float32 ulp, so only a rounding boundary can move the result).
The gather is byte-exact."""
import numpy as np
import pytest
import torch

from srl_amd import hip
from srl_amd.runtime import replay

pytestmark = pytest.mark.gpu

GUARD = 4
SENTINEL = -7.25


class Trees:
    """Both trees, the scratch and the state block on the device, each between guard elements."""

    def __init__(self, capacity, max_priority=1.0):
        dev = "cuda"
        self.capacity = capacity
        self.raw = [torch.full((GUARD + 2 * capacity + GUARD,), SENTINEL, dtype=torch.float64, device=dev) for _ in range(2)]
        self.sum, self.min = (r[GUARD:GUARD + 2 * capacity] for r in self.raw)
        self.sum.zero_()
        self.min.fill_(float("inf"))
        self.raw_last = torch.full((GUARD + capacity + GUARD,), -77, dtype=torch.int32, device=dev)
        self.last = self.raw_last[GUARD:GUARD + capacity]
        self.last.fill_(-1)
        self.state = torch.zeros(2, dtype=torch.int32, device=dev)
        self.max_priority, self.refused = self.state[:1].view(torch.float32), self.state[1:]
        self.max_priority.fill_(max_priority)

    def set(self, slots, priorities, alpha, n_slots):
        hip.per_set(self.sum, self.min, self.capacity, n_slots, torch.from_numpy(np.asarray(slots, np.int32)).cuda(),
                    torch.from_numpy(np.asarray(priorities, np.float32)).cuda(), alpha, self.last, self.max_priority, self.refused)

    def fetch(self):
        for r in self.raw:
            g = r.cpu().numpy()
            assert (g[:GUARD] == SENTINEL).all() and (g[-GUARD:] == SENTINEL).all(), "tree guard elements"
        gl = self.raw_last.cpu().numpy()
        assert (gl[:GUARD] == -77).all() and (gl[-GUARD:] == -77).all() and (gl[GUARD:-GUARD] == -1).all(), "scratch guards / reset"
        return self.sum.cpu().numpy(), self.min.cpu().numpy()


def ulp64(a, b):
    return np.abs(np.asarray(a, np.float64).view(np.int64) - np.asarray(b, np.float64).view(np.int64))


def ulp32(a, b):
    return np.abs(np.asarray(a, np.float32).view(np.int32).astype(np.int64) - np.asarray(b, np.float32).view(np.int32).astype(np.int64))


def assert_invariants(s, m):
    """Every inner node is the exact float64 sum / min of its own two children."""
    cap = s.size // 2
    node = np.arange(1, cap)
    assert np.array_equal(s[node], s[2 * node] + s[2 * node + 1]), "sum tree inner nodes"
    assert np.array_equal(m[node], np.minimum(m[2 * node], m[2 * node + 1])), "min tree inner nodes"
    assert s[0] == 0.0 and m[0] == np.inf


# (capacity, max_size, n): every n at capacity 2048; forced duplicates at max_size 5; the smallest trees with n past the capacity
SET_CASES = [(2048, 2048, n) for n in (1, 3, 64, 65, 300, 1500)] + [(8, 5, 300), (1, 1, 3), (2, 2, 3), (2, 2, 1), (131072, 131072, 1500)]


def pairs(capacity, max_size, n, seed=0):
    rng = np.random.default_rng(1000 * n + capacity + seed)
    slots = rng.integers(0, max_size, size=n).astype(np.int32)
    if n >= 3:
        slots[-1] = slots[0]  # a repeat whatever the draw: the last one must stand
    return slots, (rng.random(n) * 5 + 0.01).astype(np.float32)


@pytest.mark.parametrize("alpha", [1.0, 0.0, 0.6])
@pytest.mark.parametrize("capacity,max_size,n", SET_CASES)
def test_set(capacity, max_size, n, alpha):
    t = Trees(capacity)
    # a populated tree first (every slot, one call: more pairs than threads at the larger sizes), then the case's pairs on top
    base = (np.random.default_rng(capacity).random(max_size) * 2 + 0.5).astype(np.float32)
    t.set(np.arange(max_size), base, alpha, max_size)
    slots, pri = pairs(capacity, max_size, n)
    t.set(slots, pri, alpha, max_size)
    s, m = t.fetch()
    hs, hm = np.zeros(2 * capacity), np.full(2 * capacity, np.inf)
    hs[capacity:capacity + max_size] = hm[capacity:capacity + max_size] = replay.leaf_values(base, alpha)
    for sl, v in zip(slots, replay.leaf_values(pri, alpha)):  # the last occurrence of a slot stands
        hs[capacity + sl] = hm[capacity + sl] = v
    assert np.array_equal(np.where(np.isinf(m[capacity:]), 0.0, m[capacity:]), s[capacity:])  # one leaf value in both trees
    if alpha in (0.0, 1.0):
        # the host's own trees: the populated one bottom-up (the same sums: a node is its left child + its right one), then the
        # case's pairs the reference's way
        rs, rm = np.zeros(2 * capacity), np.full(2 * capacity, np.inf)
        rs[capacity:capacity + max_size] = rm[capacity:capacity + max_size] = replay.leaf_values(base, alpha)
        level = capacity // 2
        while level >= 1:
            node = np.arange(level, 2 * level)
            rs[node], rm[node] = rs[2 * node] + rs[2 * node + 1], np.minimum(rm[2 * node], rm[2 * node + 1])
            level //= 2
        replay.set_leaves(rs, rm, slots, replay.leaf_values(pri, alpha))
        assert np.array_equal(s, rs) and np.array_equal(m, rm)
    else:
        worst = ulp64(s[capacity:capacity + max_size], hs[capacity:capacity + max_size]).max()
        print(f"capacity {capacity} n {n}: largest leaf distance to numpy pow {worst} ulp")
        assert worst <= 16
        assert np.array_equal(s[capacity + max_size:], hs[capacity + max_size:]) and np.array_equal(m[capacity + max_size:], hm[capacity + max_size:])
        if n >= 3 and pri[0] != pri[-1]:  # the repeated slot holds its last pair's leaf, not its first's
            first, last = replay.leaf_values(pri[:1], alpha)[0], replay.leaf_values(pri[-1:], alpha)[0]
            got = s[capacity + slots[0]]
            assert ulp64(got, last) <= 16 and ulp64(got, first) > 16
    assert_invariants(s, m)
    assert t.refused.item() == 0
    assert t.max_priority.item() == max(np.float32(1.0), base.max(), pri.max())


def test_set_refuses_and_counts():
    cap, max_size = 8, 5
    t = Trees(cap, max_priority=6.0)
    base = np.array([1.0, 2.0, 3.0, 4.0, 5.0], np.float32)
    t.set(np.arange(5), base, 1.0, max_size)
    #        ok   NaN     zero  negative  +inf    slot out of range   slot < 0   ok, then refused for the same slot
    slots = [0, 1, 2, 3, 1, 5, -1, 4, 4, 7]
    pri = [0.5, np.nan, 0.0, -3.0, np.inf, 9.0, 9.0, 0.25, np.nan, 99.0]
    t.set(slots, pri, 1.0, max_size)
    s, m = t.fetch()
    want = np.array([0.5, 2.0, 3.0, 4.0, 0.25, 0.0, 0.0, 0.0])
    assert np.array_equal(s[cap:], want), s[cap:]
    assert np.array_equal(m[cap:], np.where(want > 0, want, np.inf))
    assert_invariants(s, m)
    assert t.refused.item() == 8
    assert t.max_priority.item() == 6.0  # refused priorities (9, 99, +inf) do not raise it
    # a whole call of refused pairs, more of them than threads: nothing moves
    t.set(np.zeros(1500, np.int32), np.full(1500, np.nan, np.float32), 1.0, max_size)
    s2, m2 = t.fetch()
    assert np.array_equal(s2, s) and np.array_equal(m2, m) and t.refused.item() == 1508


def test_set_takes_the_priority_from_max_priority_itself():
    """A sample without analyzed_result.ret enters with the running max_priority, read where it lives."""
    t = Trees(8, max_priority=3.5)
    hip.per_set(t.sum, t.min, 8, 1, torch.zeros(1, dtype=torch.int32, device="cuda"), t.max_priority, 1.0, t.last, t.max_priority, t.refused)
    s, m = t.fetch()
    assert s[8] == 3.5 and m[8] == 3.5 and s[1] == 3.5 and m[1] == 3.5 and t.max_priority.item() == 3.5 and t.refused.item() == 0


# ------------------------------------------------------------------------------------------------ sample
# (capacity, max_size, n_filled, B)
SAMPLE_CASES = [(2048, 2048, 2000, B) for B in (1, 3, 64, 65, 300, 1500)] + [(8, 5, 5, 300), (1, 1, 1, 3), (2, 2, 2, 3), (2, 2, 1, 1),
                                                                             (131072, 131072, 131072, 300)]


def draw(t, n_filled, B, beta, seed, offset):
    idx = torch.full((GUARD + B + GUARD,), -5, dtype=torch.int32, device="cuda")
    w = torch.full((GUARD + B + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    hip.per_sample(t.sum, t.min, t.capacity, n_filled, beta, seed, offset, idx[GUARD:GUARD + B], w[GUARD:GUARD + B])
    idx, w = idx.cpu().numpy(), w.cpu().numpy()
    assert (idx[:GUARD] == -5).all() and (idx[-GUARD:] == -5).all() and (w[:GUARD] == SENTINEL).all() and (w[-GUARD:] == SENTINEL).all()
    return idx[GUARD:-GUARD], w[GUARD:-GUARD]


@pytest.mark.parametrize("capacity,max_size,n_filled,B", SAMPLE_CASES)
def test_sample(capacity, max_size, n_filled, B):
    t = Trees(capacity)
    pri = (np.random.default_rng(B + capacity).random(n_filled) * 5 + 0.01).astype(np.float32)
    t.set(np.arange(n_filled), pri, 0.6, max_size)
    s, m = t.fetch()
    for offset, beta in ((0, 0.4), (3, 1.0)):
        seed = 0x1234567 + (B << 33)
        idx, w = draw(t, n_filled, B, beta, seed, offset)
        want_idx, want_w, _ = replay.sample_proportional(s, m, n_filled, B, beta, seed, offset)  # on the device's own tree
        assert np.array_equal(idx, want_idx), np.flatnonzero(idx != want_idx)[:8]
        assert (np.diff(idx) >= 0).all() and idx.min() >= 0 and idx.max() <= n_filled - 1
        worst = ulp32(w, want_w).max()
        print(f"capacity {capacity} B {B} beta {beta}: largest weight distance {worst} float32 ulp")
        assert worst <= 1 and np.isfinite(w).all() and (w > 0).all() and (w <= 1.0).all()
    if B >= 64:
        assert not np.array_equal(idx, draw(t, n_filled, B, 0.4, seed, 0)[0])  # another offset, other draws


def test_sample_masses_exactly_on_leaf_boundaries():
    """total = B and a boundary at every draw's mass: leaves u_0, 1 - u_0, u_1, 1 - u_1, ... (multiples of 2^-24 below 1: exact in
    float32; every partial sum exact in float64).  Then range = 1, mass_i = u_i + i is the prefix sum of leaves 0 .. 2 i, and
    find_prefixsum_idx takes the leaf to the RIGHT of a boundary it sits on: idx_i = 2 i + 1."""
    B, seed, offset = 64, 99, 5
    u = replay.stratified_uniforms(B, seed, offset)
    assert (u > 0).all()
    leaves = np.stack([u, 1.0 - u], 1).reshape(-1).astype(np.float32)
    assert np.array_equal(leaves.astype(np.float64), np.stack([u, 1.0 - u], 1).reshape(-1))
    t = Trees(2048)
    t.set(np.arange(2 * B), leaves, 1.0, 2048)
    s, m = t.fetch()
    assert s[1] == float(B)
    want_idx, want_w, mass = replay.sample_proportional(s, m, 2 * B, B, 0.4, seed, offset)
    assert np.array_equal(mass, np.cumsum(leaves.astype(np.float64))[0::2]) and np.array_equal(want_idx, 2 * np.arange(B) + 1)
    idx, w = draw(t, 2 * B, B, 0.4, seed, offset)
    assert np.array_equal(idx, want_idx) and (ulp32(w, want_w) <= 1).all()


def test_sample_clamps_to_the_filled_slots():
    """A walk that ends past the filled slots -- what a mass equal to the root does (tests/test_replay_host.py) -- is clamped to the last
    filled one, whose leaf gives the weight: here the tree holds mass in five leaves and three count as filled."""
    t = Trees(8)
    t.set(np.arange(5), np.array([1, 2, 3, 4, 5], np.float32), 1.0, 5)
    s, m = t.fetch()
    idx, w = draw(t, 3, 65, 0.4, 7, 0)
    want_idx, want_w, mass = replay.sample_proportional(s, m, 3, 65, 0.4, 7, 0)
    assert (replay.find_prefixsum_idx(s, mass) > 2).any() and idx.max() == 2
    assert np.array_equal(idx, want_idx) and (ulp32(w, want_w) <= 1).all() and np.isfinite(w).all()


# ------------------------------------------------------------------------------------------------ gather
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("B", [1, 65])
@pytest.mark.parametrize("Tb", [1, 3])
@pytest.mark.parametrize("row_bytes,misalign", [(4, 0), (20, 0), (28224, 0), (2048, 4)])
def test_gather(row_bytes, misalign, Tb, B, dtype):
    max_size = 7
    rng = np.random.default_rng(row_bytes + 10 * Tb + B)
    host = rng.integers(0, 256, size=(max_size, Tb, row_bytes), dtype=np.uint8)
    if dtype is np.float32:
        host = rng.normal(size=(max_size, Tb, row_bytes // 4)).astype(np.float32).view(np.uint8).reshape(max_size, Tb, row_bytes)
    n = host.size
    raw_store = torch.zeros(misalign + n + 16, dtype=torch.uint8, device="cuda")
    store = raw_store[misalign:misalign + n]
    store.copy_(torch.from_numpy(host.reshape(-1)))
    idx = rng.integers(0, max_size, size=B).astype(np.int32)
    idx[0] = max_size - 1
    pad = 64  # guard bytes around the destination (a multiple of 16: the destination keeps the store's alignment class)
    out_n = Tb * B * row_bytes
    raw_dst = torch.full((pad + misalign + out_n + pad,), 0xA5, dtype=torch.uint8, device="cuda")
    dst = raw_dst[pad + misalign:pad + misalign + out_n]
    assert store.data_ptr() % 16 == misalign and dst.data_ptr() % 16 == misalign
    hip.replay_gather(store.data_ptr(), max_size, torch.from_numpy(idx).cuda(), B, Tb, row_bytes, dst.data_ptr())
    got = raw_dst.cpu().numpy()
    want = np.swapaxes(host[idx], 0, 1).reshape(-1)
    assert np.array_equal(got[pad + misalign:pad + misalign + out_n], want)
    assert (got[:pad + misalign] == 0xA5).all() and (got[pad + misalign + out_n:] == 0xA5).all(), "destination padding"


def test_gather_leaves_rows_of_a_slot_outside_the_store_alone():
    max_size, Tb, B, row = 3, 2, 4, 2048
    host = np.random.default_rng(0).integers(0, 256, size=(max_size, Tb, row), dtype=np.uint8)
    store = torch.from_numpy(host).cuda()
    for rb in (row, 20):  # both kernels
        st = store[:, :, :rb].contiguous()
        dst = torch.full((Tb, B, rb), 0xA5, dtype=torch.uint8, device="cuda")
        idx = np.array([2, 3, -1, 0], np.int32)
        hip.replay_gather(st.data_ptr(), max_size, torch.from_numpy(idx).cuda(), B, Tb, rb, dst.data_ptr())
        got = dst.cpu().numpy()
        assert np.array_equal(got[:, 0], host[2, :, :rb]) and np.array_equal(got[:, 3], host[0, :, :rb]) and (got[:, 1:3] == 0xA5).all()


# ------------------------------------------------------------------------------------------------ the step's means
def test_pairwise_means_are_numpys_float32_means():
    rng = np.random.default_rng(5)
    out = torch.zeros(3, dtype=torch.float64, device="cuda")
    sizes = [1, 2, 3, 7, 8, 9, 15, 16, 17, 64, 65, 127, 128, 129, 130, 255, 257, 300, 1500, 7680]
    for k in range(0, len(sizes), 2):
        a, b = ((rng.random(n) * 3).astype(np.float32) for n in sizes[k:k + 2])
        hip.pairwise_means([torch.from_numpy(a).cuda(), None, torch.from_numpy(b).cuda()], out)
        got = out.cpu().numpy()
        assert got[0] == float(a.mean()) and got[1] == 0.0 and got[2] == float(b.mean()), (sizes[k:k + 2], got, a.mean(), b.mean())
    a = np.array([1.0, np.nan, 2.0], np.float32)
    hip.pairwise_means([None, torch.from_numpy(a).cuda(), None], out)
    assert np.isnan(out.cpu().numpy()[1])
