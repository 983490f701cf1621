"""The recurrent ``atari-dqn`` agent (R2D2) end to end on the device.

  * Against the REAL reference's recorded runs (tests/golden/r2d2.npz, cases and bars: tests/r2d2_cases.py): GRU with burn-in and
    two LSTM layers at hidden_dim 512, two trainer steps each -- analyze outputs, statistics, priorities, target-moved flags and
    both networks' final parameters.  No row is left out (the generator asserts the Q gap of every analysed row).
  * At hidden_dim 32 and 64 (the one-launch chunk kernels; the reference does not run there: ``rnn_towers_read_hidden_dim=True``) against the torch restatement
    tests/r2d2_ref.py in float64 under ``rnn_ref.check_vs_float64``: several chunks, ragged B = 3, burn-in in front of its chunk and
    with C != chunk_len; head outputs and ``net.grad``.
  * ``rollout``: single-step calls threading ``hx`` reproduce ``analyze`` over the same frames as one chunk; a reset row ignores its
    incoming state; ``target_value`` comes from the incoming state; the returned ``hx``.
  * The checkpoint round trip of tests/test_gpu_dqn.py."""
import numpy as np
import pytest
import torch

import dqn_ref
import r2d2_ref
import srl_amd
from dqn_cases import assert_within
from r2d2_cases import ACT, B, PARAM_TOL, RUNS, bar_scale, e2e_arrays, rel_err, unpack_params
from rnn_ref import check_vs_float64
from srl_amd.api import config, policy as policy_api, trainer as trainer_api
from srl_amd.api.env_utils import DiscreteAction
from srl_amd.api.trainer import SampleBatch
from srl_amd.algorithm.dqn_policy import DQNPolicyState
from srl_amd.namedarray import NamedArray
from srl_amd.runtime import synthetic

pytestmark = pytest.mark.gpu
srl_amd.register_all()


@pytest.fixture(scope="module")
def g(golden):
    return golden("r2d2.npz")


def to_sample(a, weighted=False):
    return SampleBatch(obs=NamedArray(obs=a["obs.obs"]), policy_state=DQNPolicyState(hx=a["policy_state.hx"], epsilon=a["policy_state.epsilon"]),
                       on_reset=a["on_reset"], done=a["done"], truncated=a["truncated"], action=DiscreteAction(a["action.x"]),
                       reward=a["reward"], info_mask=a["info_mask"], sampling_weight=a["sampling_weight"] if weighted else None)


def make_trainer(run, **policy):
    r = RUNS[run]
    return trainer_api.make(config.Trainer("q-learning", args=r["trainer"]), config.Policy("atari-dqn", args=dict(r["policy"], **policy)))


def state(trainer):
    return {k: v.numpy() for k, v in trainer.policy.get_checkpoint()["state_dict"].items()}


def gathered(out):
    """``q_tot`` / ``target_q_tot`` of the head outputs, as the reference gathers them (atari_dqn_policy.py:218-231)."""
    n = out.T * out.B
    q_on = dqn_ref.dueling_q(out.adv.cpu().numpy(), out.value.cpu().numpy(), np.float32)
    q_tg = dqn_ref.dueling_q(out.target_adv.cpu().numpy(), out.target_value.cpu().numpy(), np.float32)
    rows = np.arange(n)
    return q_on[rows, out.action.cpu().numpy()], q_tg[rows, q_on.argmax(-1)]


@pytest.mark.parametrize("run", list(RUNS))
def test_two_steps_match_the_reference(g, run):
    r = RUNS[run]
    weighted, burn = bool(r["trainer"].get("use_priority_weight")), r["trainer"].get("burn_in_steps", 0)
    trainer = make_trainer(run)
    policy = trainer.policy
    init = state(trainer)
    names = [str(k) for k in g[f"{run}_stat_names"]]
    for step in range(2):
        sample = to_sample(e2e_arrays(run, step), weighted)
        if step == 0:
            out = policy.analyze(sample, target="dqn", burn_in_steps=burn)
            n = out.T * out.B
            for k, got in zip(("q_tot", "target_q_tot"), gathered(out)):
                err, bar = rel_err(got, g[f"{run}_{k}"].reshape(n), 1e-3), 1e-5 * bar_scale(g, run, k)
                print(f"{run} {k}: {err:.3e} (bar {bar:.3e})")
                assert err <= bar, (run, k, err, bar)
        before = state(trainer)
        res = trainer.step(sample)
        want = dict(zip(names, g[f"{run}_stats{step}"]))
        assert set(res.stats) == set(names), set(res.stats) ^ set(names)
        bar = 1e-5 * bar_scale(g, run, f"stats{step}")
        for k in names:
            print(f"{run} step {step} {k}: {res.stats[k]!r} (reference {want[k]!r})")
        for k in names:
            assert rel_err(res.stats[k], want[k], 1e-2) <= bar, (run, step, k, res.stats[k], want[k])
        assert res.step == int(g[f"{run}_step{step}"]) == step + 1 and policy.version == step
        pri = g[f"{run}_priorities{step}"].reshape(-1)
        assert res.priorities.shape == pri.shape
        assert rel_err(res.priorities, pri, 1e-3) <= 1e-5 * bar_scale(g, run, f"priorities{step}"), (res.priorities, pri)
        after = state(trainer)
        moved = any(not np.array_equal(after[k], before[k]) for k in after if k.startswith("target_net."))
        assert moved == bool(g[f"{run}_target_moved{step}"])
        if run == "gru" and step == 1:  # the hard update: an exact copy
            assert all(np.array_equal(after["target_" + k], v) for k, v in after.items() if k.startswith("net."))
    worst, tol = (0.0, ""), PARAM_TOL * bar_scale(g, run, "params")
    for k, (want_v, q, idx) in unpack_params(g, f"{run}_final", init).items():
        err = np.abs(after[k].reshape(-1).astype(np.float64)[idx] - want_v).max()
        worst = max(worst, (err, k))
        assert err <= tol - q, (run, k, err, q)
    print(f"{run}: largest parameter difference after two steps {worst[0]:.3e} at {worst[1]}")
    assert len(trainer.optimizer.state_dict()["state"]) == int(g[f"{run}_optim_state_params"])


# (rnn_type, hidden_dim, layers, chunk_len, burn, Tb): the chunk kernels' widths; two chunks each; the second case has 10 analysed
# steps with chunk_len 4 -- two chunks of 5, the second burn-in window not in front of its chunk
SMALL = [("gru", 32, 1, 4, 2, 10), ("lstm", 64, 2, 4, 2, 12), ("lstm", 32, 1, 3, 0, 6), ("gru", 64, 2, 2, 3, 7)]


@pytest.mark.parametrize("kind,H,layers,cl,burn,Tb", SMALL, ids=lambda v: str(v))
def test_small_widths_vs_float64_restatement(kind, H, layers, cl, burn, Tb):
    pargs = dict(act_dim=ACT, dueling=True, chunk_len=cl, seed=3 + H, hidden_dim=H, num_rnn_layers=layers, rnn_type=kind,
                 rnn_towers_read_hidden_dim=True)
    policy = policy_api.make(config.Policy("atari-dqn", args=pargs))
    SW = H * (2 if kind == "lstm" else 1)
    arrays = synthetic.make_sample_arrays(seed=Tb + H, T=Tb - 1, B=B, obs_spec={"obs": ((4, 84, 84), "u8")}, action_dims=ACT, p_done=0.25,
                                          bootstrap_steps=1, policy_state={"hx": (layers, SW)})
    assert arrays["on_reset"][burn:].any()
    arrays["policy_state.epsilon"] = np.ones((Tb, B, 1), np.float32)
    sd = {k: v.numpy() for k, v in policy.get_checkpoint()["state_dict"].items()}
    rng = np.random.default_rng(H)
    T = Tb - burn
    d_adv, d_v = rng.standard_normal((T * B, ACT)).astype(np.float32), rng.standard_normal((T * B, 1)).astype(np.float32)
    policy.net.zero_grad()
    out = policy.analyze(to_sample(arrays), target="dqn", burn_in_steps=burn)
    assert (out.T, out.B) == (T, B)
    got = {k: getattr(out, f).cpu().numpy().astype(np.float64) for k, f in (("adv", "adv"), ("v", "value"), ("tadv", "target_adv"), ("tv", "target_value"))}
    policy.backward_dqn(torch.from_numpy(d_adv).to(policy.device), torch.from_numpy(d_v).to(policy.device))
    grads = policy.net.flat_to_reference(policy.net.grad.detach().cpu())
    stats = dict(loss=float((got["adv"] * d_adv).sum() + (got["v"] * d_v).sum()))
    oracles, heads = {}, {}
    for dt in (torch.float32, torch.float64):
        net, target = (r2d2_ref.make_net(sd, p, pargs, dt) for p in ("net.", "target_net."))
        ref = r2d2_ref.analyze(net, target, arrays, burn, cl, dt)
        loss = (ref["adv"].reshape(T * B, ACT) * torch.from_numpy(d_adv).to(dt)).sum() + (ref["v"].reshape(T * B, 1) * torch.from_numpy(d_v).to(dt)).sum()
        loss.backward()
        net.params = dict(net.named_parameters())
        oracles[dt] = (net, dict(loss=float(loss.detach())))
        heads[dt] = {k: ref[k].detach().reshape(T * B, -1).numpy() for k in got}
    assert set(grads) == set(oracles[torch.float64][0].params)
    for k in got:
        worst = assert_within(k, got[k], heads[torch.float32][k], heads[torch.float64][k])
        print(f"{k}: worst error / bound {worst:.3f}")
    check_vs_float64(stats, grads, oracles, ("loss",))


ROLL = dict(act_dim=ACT, dueling=True, chunk_len=4, seed=21, hidden_dim=32, num_rnn_layers=2, rnn_type="lstm",
            rnn_towers_read_hidden_dim=True)


def request(frames, hx, on_reset, is_eval):
    n = frames.shape[0]
    eps = np.zeros((n, 1), np.float32)
    return policy_api.RolloutRequest(obs=NamedArray(obs=frames, epsilon=eps), is_evaluation=is_eval, on_reset=on_reset,
                                     policy_state=DQNPolicyState(hx=hx, epsilon=eps))


def close(got, want):
    """1e-5 of the tensor's largest magnitude: single-step calls and one chunk of four sum the same float32 terms in another order."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return bool((np.abs(got - want) <= 1e-5 * np.abs(want).max()).all())


def test_rollout_threads_the_state_like_one_chunk():
    n, T = 5, 4
    rng = np.random.default_rng(8)
    frames = rng.integers(0, 256, size=(T, n, 4, 84, 84), dtype=np.uint8)
    on_reset = np.zeros((T, n, 1), np.uint8)
    on_reset[2, 1] = on_reset[2, 3] = on_reset[0, 4] = 1   # mid-way, and on the first step over a non-zero state
    policy = policy_api.make(config.Policy("atari-dqn", args=ROLL))
    L, SW = 2, 64
    hx0 = (0.3 * rng.standard_normal((n, L, SW))).astype(np.float32)
    ones = np.ones((n, 1), np.uint8)
    hx, actions, values, targets = hx0, [], [], []
    for t in range(T):
        res = policy.rollout(request(frames[t], hx, on_reset[t], ones))
        hx = res.policy_state.hx
        assert hx.shape == (n, L, SW) and hx.dtype == np.float32
        assert res.action.x.shape == (n, 1) and res.action.x.dtype == np.int64
        actions.append(res.action.x), values.append(res.analyzed_result.value), targets.append(res.analyzed_result.target_value)
    stored = np.zeros((T, n, L, SW), np.float32)
    stored[0] = hx0
    sample = SampleBatch(obs=NamedArray(obs=frames), on_reset=on_reset, action=DiscreteAction(np.stack(actions).astype(np.int32)),
                         policy_state=DQNPolicyState(hx=stored, epsilon=np.zeros((T, n, 1), np.float32)))
    out = policy.analyze(sample, target="dqn")
    q_tot, target = gathered(out)
    greedy = dqn_ref.dueling_q(out.adv.cpu().numpy(), out.value.cpu().numpy(), np.float32).argmax(-1)
    assert np.array_equal(np.stack(actions).reshape(-1), greedy)   # every row is an evaluation row
    assert close(np.stack(values).reshape(-1), q_tot), np.abs(np.stack(values).reshape(-1) - q_tot).max()
    assert close(np.stack(targets).reshape(-1), target)
    assert close(hx, policy.net.last_state["a:"].permute(1, 0, 2).cpu().numpy())   # the chunk's final state


def test_rollout_reset_rows_and_the_target_s_state():
    n = 6
    rng = np.random.default_rng(9)
    frames = rng.integers(0, 256, size=(n, 4, 84, 84), dtype=np.uint8)
    on_reset = (np.arange(n) % 2).astype(np.uint8).reshape(n, 1)
    ones = np.ones((n, 1), np.uint8)
    policy = policy_api.make(config.Policy("atari-dqn", args=ROLL))
    ha, hb = ((0.5 * rng.standard_normal((n, 2, 64))).astype(np.float32) for _ in range(2))
    ra, rb = policy.rollout(request(frames, ha, on_reset, ones)), policy.rollout(request(frames, hb, on_reset, ones))
    rs = on_reset.reshape(n) != 0
    for a, b in ((ra.analyzed_result.value, rb.analyzed_result.value), (ra.analyzed_result.target_value, rb.analyzed_result.target_value),
                 (ra.policy_state.hx, rb.policy_state.hx)):
        assert np.array_equal(a[rs], b[rs])            # a reset row ignores its incoming state
        assert not np.array_equal(a[~rs], b[~rs])      # the others carry it
    # the target network is a copy of the online one here: from the INCOMING state it values the greedy action exactly as the online
    # network does; from the online network's new state it would not
    assert close(ra.analyzed_result.target_value, ra.analyzed_result.value)
    zero = policy.rollout(request(frames, np.zeros_like(ha), on_reset, ones))
    assert np.array_equal(zero.analyzed_result.value[rs], ra.analyzed_result.value[rs])
    with pytest.raises(ValueError):
        policy.rollout(policy_api.RolloutRequest(obs=NamedArray(obs=frames, epsilon=np.zeros((n, 1), np.float32)), is_evaluation=ones))


def test_checkpoint_round_trip_restores_both_nets_and_the_optimiser(g):
    run = "gru"
    a = make_trainer(run)
    a.step(to_sample(e2e_arrays(run, 0)))
    ckpt = a.get_checkpoint()
    assert list(ckpt["state_dict"]) == [str(k) for k in g["table_gru1_names"]]  # the reference's layout
    b = make_trainer(run, seed=RUNS[run]["policy"]["seed"] + 1)
    key = "net.rnn._AutoResetRNN__net.weight_ih_l0"
    assert not np.array_equal(state(b)[key], state(a)[key])
    b.load_checkpoint(ckpt)
    sa, sb = state(a), state(b)
    assert all(np.array_equal(sa[k], sb[k]) for k in sa) and b.policy.version == a.policy.version
    oa, ob = a.optimizer.state_dict(), b.optimizer.state_dict()
    assert oa["param_groups"] == ob["param_groups"] and set(oa["state"]) == set(ob["state"])
    for i, st in oa["state"].items():
        assert all(torch.equal(v, ob["state"][i][k]) for k, v in st.items())
    b.steps, b.last_hard_update_step, b.hard_update_count = a.steps, a.last_hard_update_step, a.hard_update_count
    # ... and the restored trainer continues as the original does.  Not bit for bit at this size: the trunk's bias gradients are
    # summed with atomics, and two runs of the SAME step on the same state differ in conv1.bias's gradient by up to 2e-9 (of 2e-2;
    # measured, with and without the second stream).  A moment or a parameter restored wrongly moves weights by a fraction of an
    # optimiser step (5e-4, dqn_cases.PARAM_TOL = 4 % of it); a last-bit difference of a gradient moves them by 1e-7 of a step.
    # The bar is a hundredth of PARAM_TOL.
    ra, rb = a.step(to_sample(e2e_arrays(run, 1))), b.step(to_sample(e2e_arrays(run, 1)))
    for k in ("value_loss", "grad_norm", "max_td_err"):
        assert abs(ra.stats[k] - rb.stats[k]) <= 1e-6 * abs(ra.stats[k]), (k, ra.stats[k], rb.stats[k])
    sa, sb = state(a), state(b)
    worst = max((float(np.abs(sa[k].astype(np.float64) - sb[k]).max()), k) for k in sa)
    print(f"continued step: largest parameter difference {worst[0]:.3e} at {worst[1]}")
    assert worst[0] <= PARAM_TOL / 100, worst
