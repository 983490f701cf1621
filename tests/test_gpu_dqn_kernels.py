"""The deep Q-learning kernels (csrc/dqn.hip; the value loss and the sampler's Philox draw are csrc/action_dist.h's, shared with
the PPO loss and the action heads) against the float64 restatements of tests/dqn_ref.py.

TD step: every element of d_adv, d_v, the priorities and the statistics obeys the project's rule (dqn_cases.assert_within: three times
the float32 reference's own error plus 2e-6 of the tensor's largest element), in every case of dqn_cases.TD_CASES and every variant
of dqn_cases.TD_VARIANTS; the head outputs and the gradient sit in wider buffers whose padding must stay as it was.
Sampler: bit-exact actions, values and target values.  Polyak: tau = 1 copies bit for bit, tau = 0.005 obeys the rule."""
import numpy as np
import pytest
import torch

import dqn_ref
from dqn_cases import DELTA, TD_CASES, TD_VARIANTS, assert_within, grid, td_case, td_ref
from srl_amd import hip

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAD, SENTINEL = 3, 7.0


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).to(DEV)


def padded(x, fill=np.nan):
    """[rows, A] as a window of a [rows, A + PAD] device matrix filled with `fill`."""
    wide = np.full((x.shape[0], x.shape[1] + PAD), fill, np.float32)
    wide[:, :x.shape[1]] = x
    t = dev(wide)
    return t, t[:, :x.shape[1]]


def hparams(c, variant, gamma=0.99, eta=0.9, eps=1e-3):
    ast, dq, loss, _ = variant
    return hip.DqnHparams(gamma=gamma, scalar_transform_eps=eps, priority_interpolation_eta=eta, huber_delta=DELTA, n=c["n"],
                          apply_scalar_transform=int(ast), double_q=int(dq), value_loss=hip.VALUE_LOSS_KINDS[loss])


@pytest.mark.parametrize("case", TD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_td_step_matches_float64(case):
    c = td_case(*case)
    T, B, A, S = c["T"], c["B"], c["A"], c["S"]
    assert (len(c["all_done"]) >= 1) == (B >= 2)
    adv_buf, adv = padded(c["adv"])
    tadv_buf, tadv = padded(c["tadv"])
    v, tv, action, reward, done, trunc, weight = (dev(c[k]) for k in ("v", "tv", "action", "reward", "done", "truncated", "weight"))
    worst = 0.0
    for variant in TD_VARIANTS:
        r32, r64 = td_ref(c, variant, np.float32), td_ref(c, variant, np.float64)
        assert np.array_equal(r32["greedy"], r64["greedy"])  # the grid: both precisions see the same ties
        d_buf = torch.full((T * B, A + PAD), SENTINEL, device=DEV)
        d_adv = d_buf[:, :A]
        d_v = torch.full((T * B,), SENTINEL, device=DEV)
        terms = torch.full((hip.DQ_COUNT,), SENTINEL, dtype=torch.float64, device=DEV)
        pri = torch.full((B,), SENTINEL, device=DEV)
        hip.dqn_td_fwd_bwd(adv, v, tadv, tv, action, reward, done, trunc, weight if variant[3] else None, T, B,
                           hparams(c, variant), d_adv, d_v, terms, pri)
        torch.cuda.synchronize()
        g_adv, g_v, g_terms, g_pri = d_buf.cpu().numpy(), d_v.cpu().numpy(), terms.cpu().numpy(), pri.cpu().numpy()
        assert (g_adv[:, A:] == SENTINEL).all(), "the gradient's padding was written"
        assert np.isnan(adv_buf.cpu().numpy()[:, A:]).all() and np.isnan(tadv_buf.cpu().numpy()[:, A:]).all()
        g_adv = g_adv[:, :A]
        assert not g_adv[S * B:].any() and not g_v[S * B:].any(), "rows t >= S must be exactly zero"
        worst = max(worst, assert_within("d_adv", g_adv, r32["d_adv"], r64["d_adv"]),
                    assert_within("d_v", g_v, r32["d_v"], r64["d_v"]),
                    assert_within("priorities", g_pri, r32["priorities"], r64["priorities"]))
        for i, k in enumerate(dqn_ref.TERMS):
            worst = max(worst, assert_within(k, g_terms[i], r32["terms"][k], r64["terms"][k]))
        # the all-done column: NaN priority on both sides (assert_within), everything else finite
        assert np.array_equal(np.flatnonzero(np.isnan(g_pri)), c["all_done"])
        assert np.isfinite(g_adv).all() and np.isfinite(g_v).all() and np.isfinite(g_terms).all()
        # rows of d_adv sum to zero: A roundings of g (1[a == action] - 1/A) and of their sum, 1/A rounded once
        rowsum = np.abs(g_adv.astype(np.float64).sum(1))
        assert (rowsum <= (2 * A + 4) * 2.0**-24 * np.abs(g_v)).all(), float(rowsum.max())
    print(f"\n{case}: worst error / bound {worst:.3f}")


def test_td_step_refuses_bad_shapes():
    c = td_case(2, 1, 2, 1)
    t = {k: dev(c[k]) for k in ("adv", "tadv", "v", "tv", "action", "reward", "done", "truncated")}
    out = (torch.zeros(2, 2, device=DEV), torch.zeros(2, device=DEV), torch.zeros(hip.DQ_COUNT, dtype=torch.float64, device=DEV),
           torch.zeros(1, device=DEV))
    hp = hparams(c, TD_VARIANTS[0])
    hp.n = 2  # no loss row left
    with pytest.raises(hip.HipError):
        hip.dqn_td_fwd_bwd(t["adv"], t["v"], t["tadv"], t["tv"], t["action"], t["reward"], t["done"], t["truncated"], None, 2, 1, hp, *out)


# ------------------------------------------------------------------------------------------------ sampler
N_ROWS = 130


@pytest.mark.parametrize("A", [6, 18])
@pytest.mark.parametrize("eps_kind", ["zero", "one", "per-row"])
@pytest.mark.parametrize("double_q", [True, False])
def test_epsilon_greedy_sampler_is_bit_exact(A, eps_kind, double_q):
    rng = np.random.default_rng(A)
    n = N_ROWS
    adv, tadv, v, tv = grid(rng, (n, A)), grid(rng, (n, A)), grid(rng, (n,)), grid(rng, (n,))
    adv[5, :] = 1.0  # every action ties: the first wins
    eps = dict(zero=np.zeros(n), one=np.ones(n))[eps_kind] if eps_kind != "per-row" else rng.random(n)
    eps = eps.astype(np.float32)
    is_eval = (rng.random(n) < 0.3).astype(np.uint8)
    seed, offset, row0 = 0x1234_5678_9ABC_DEF0, 0x1_0000_0007, 0xFFFF_FFF0  # the rows cross a carry into the counter's second word
    adv_buf, adv_d = padded(adv)
    tadv_buf, tadv_d = padded(tadv)
    for ev in (None, is_eval):
        want = dqn_ref.epsilon_greedy_sample(adv, v, tadv, tv, eps, ev, double_q, seed, offset, row0)
        action = torch.full((n,), -1, dtype=torch.int64, device=DEV)
        value, tvalue = torch.full((n,), SENTINEL, device=DEV), torch.full((n,), SENTINEL, device=DEV)
        hip.epsilon_greedy_sample(adv_d, dev(v), tadv_d, dev(tv), dev(eps), None if ev is None else dev(ev), double_q, seed, offset,
                                  action, value, tvalue, row0=row0)
        torch.cuda.synchronize()
        got = action.cpu().numpy()
        assert np.array_equal(got, want[0]), np.flatnonzero(got != want[0])[:8]
        assert np.array_equal(value.cpu().numpy(), want[1]) and np.array_equal(tvalue.cpu().numpy(), want[2])
        # ... and the values are the gathers at the actions it returned
        q_on, q_tg = dqn_ref.dueling_q(adv, v.reshape(-1, 1), np.float64), dqn_ref.dueling_q(tadv, tv.reshape(-1, 1), np.float64)
        greedy = q_on.argmax(-1)
        assert np.allclose(value.cpu().numpy(), q_on[np.arange(n), got], rtol=0, atol=2e-6 * 8)
        assert np.allclose(tvalue.cpu().numpy(), q_tg[np.arange(n), greedy] if double_q else q_tg.max(-1), rtol=0, atol=2e-6 * 8)
        if ev is not None:
            assert np.array_equal(got[ev != 0], greedy[ev != 0])
        if eps_kind == "zero":
            assert np.array_equal(got, greedy)
        if eps_kind == "one" and ev is None:
            assert len(set(got.tolist())) == A and (got != greedy).any()
    # another offset / row0: another stream
    if eps_kind == "one":
        other = dqn_ref.epsilon_greedy_sample(adv, v, tadv, tv, eps, None, double_q, seed, offset + 1, row0)[0]
        assert not np.array_equal(other, want[0])


# ------------------------------------------------------------------------------------------------ Polyak
@pytest.mark.parametrize("n,shift", [(5, 0), (1027, 0), (1027, 1)], ids=["5", "1027", "1027-unaligned"])
def test_polyak_update(n, shift):
    rng = np.random.default_rng(n + shift)
    target, param = rng.standard_normal(n + shift).astype(np.float32), rng.standard_normal(n + shift).astype(np.float32)
    param[:3] = [np.inf, -0.0, 1e-40]  # a copy keeps what a multiplication by zero would not (inf * 0), a signed zero, a subnormal
    t_buf, p_buf = dev(target), dev(param)
    t, p = t_buf[shift:], p_buf[shift:]
    hip.polyak_update(t, p, 1.0)
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy().view(np.uint32), param[shift:].view(np.uint32)), "tau = 1 must copy bit for bit"
    if shift:
        assert t_buf.cpu().numpy()[0] == target[0]
    param[:3] = rng.standard_normal(3)
    t_buf, p_buf = dev(target), dev(param)
    t, p = t_buf[shift:], p_buf[shift:]
    hip.polyak_update(t, p, 0.005)
    torch.cuda.synchronize()
    assert_within("polyak", t.cpu().numpy(), dqn_ref.polyak(target[shift:], param[shift:], 0.005, np.float32),
                  dqn_ref.polyak(target[shift:], param[shift:], 0.005, np.float64))
    assert np.array_equal(p.cpu().numpy(), param[shift:])
