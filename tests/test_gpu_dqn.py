"""``q-learning`` + ``atari-dqn`` end to end on the device against the REAL reference's recorded run (tests/golden/dqn.npz, written by
tests/golden/gen_dqn.py): Tb = 6, B = 3, frames 4 x 84 x 84, six actions, bootstrap_steps = 2; Adam with a hard target update that
crosses its interval, RMSprop with a soft one, sampling weights, huber loss and a clipped gradient (tests/dqn_cases.py::RUNS).

``analyze`` outputs, statistics and priorities are held at 1e-5 relative (the golden cases' bar); parameters after two steps at
``dqn_cases.PARAM_TOL`` less the fixture's encoding error.  No row is left out: the generator asserts that in every recorded row the
two largest online Q values differ by more than 1e-3 of the row's largest |Q|."""
import numpy as np
import pytest
import torch

import dqn_ref
import srl_amd
from dqn_cases import ACT, PARAM_TOL, POLICY, RUNS, e2e_arrays, unpack_params
from srl_amd.api import config, policy as policy_api, trainer as trainer_api
from srl_amd.api.env_utils import DiscreteAction
from srl_amd.api.trainer import SampleBatch
from srl_amd.algorithm.dqn_policy import DQNPolicyState
from srl_amd.namedarray import NamedArray

pytestmark = pytest.mark.gpu
srl_amd.register_all()


@pytest.fixture(scope="module")
def g(golden):
    return golden("dqn.npz")


def make_sample(step, weighted):
    a = e2e_arrays(step)
    return SampleBatch(obs=NamedArray(obs=a["obs.obs"]), policy_state=DQNPolicyState(hx=None, epsilon=a["policy_state.epsilon"]),
                       on_reset=a["on_reset"], done=a["done"], truncated=a["truncated"], action=DiscreteAction(a["action.x"]),
                       reward=a["reward"], info_mask=a["info_mask"], sampling_weight=a["sampling_weight"] if weighted else None)


def make_trainer(run):
    return trainer_api.make(config.Trainer("q-learning", args=RUNS[run]), config.Policy("atari-dqn", args=POLICY))


def close(got, want, rel=1e-5, floor=1e-2):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return bool((np.abs(got - want) <= rel * np.maximum(np.abs(want), floor)).all())


def state(trainer):
    return {k: v.numpy() for k, v in trainer.policy.get_checkpoint()["state_dict"].items()}


@pytest.mark.parametrize("run", list(RUNS))
def test_two_steps_match_the_reference(g, run):
    weighted = bool(RUNS[run].get("use_priority_weight"))
    trainer = make_trainer(run)
    policy = trainer.policy
    init = state(trainer)
    names = [str(k) for k in g[f"{run}_stat_names"]]
    for step in range(2):
        sample = make_sample(step, weighted)
        if step == 0:  # the head outputs analyze returns, gathered as the reference gathers them (atari_dqn_policy.py:218-231)
            out = policy.analyze(sample, target="dqn", burn_in_steps=0)
            n = out.T * out.B
            q_on = dqn_ref.dueling_q(out.adv.cpu().numpy(), out.value.cpu().numpy(), np.float32)
            q_tg = dqn_ref.dueling_q(out.target_adv.cpu().numpy(), out.target_value.cpu().numpy(), np.float32)
            rows = np.arange(n)
            q_tot = q_on[rows, out.action.cpu().numpy()]
            target = q_tg[rows, q_on.argmax(-1)]
            assert close(q_tot, g[f"{run}_q_tot"].reshape(n), floor=1e-3), np.abs(q_tot - g[f"{run}_q_tot"].reshape(n)).max()
            assert close(target, g[f"{run}_target_q_tot"].reshape(n), floor=1e-3)
        before = state(trainer)
        res = trainer.step(sample)
        want = dict(zip(names, g[f"{run}_stats{step}"]))
        assert set(res.stats) == set(names), set(res.stats) ^ set(names)
        for k in names:
            print(f"{run} step {step} {k}: {res.stats[k]!r} (reference {want[k]!r})")
        for k in names:
            assert close(res.stats[k], want[k]), (run, step, k, res.stats[k], want[k])
        assert res.step == int(g[f"{run}_step{step}"]) == step + 1 and policy.version == step
        pri = g[f"{run}_priorities{step}"].reshape(-1)
        assert res.priorities.shape == pri.shape and close(res.priorities, pri, floor=1e-3), (res.priorities, pri)
        # the target network changes only at its update steps
        after = state(trainer)
        moved = any(not np.array_equal(after[k], before[k]) for k in after if k.startswith("target_net."))
        assert moved == bool(g[f"{run}_target_moved{step}"])
        if run == "adam" and step == 1:  # the hard update: an exact copy
            assert all(np.array_equal(after["target_" + k], v) for k, v in after.items() if k.startswith("net."))
    worst = (0.0, "")
    for k, (want_v, q, idx) in unpack_params(g, f"{run}_final", init).items():
        got = after[k].reshape(-1).astype(np.float64)
        err = np.abs((got if idx is None else got[idx]) - want_v).max()
        worst = max(worst, (err, k))
        assert err <= PARAM_TOL - q, (run, k, err, q)
    print(f"{run}: largest parameter difference after two steps {worst[0]:.3e} at {worst[1]}")
    assert len(trainer.optimizer.state_dict()["state"]) == int(g[f"{run}_optim_state_params"])


@pytest.mark.parametrize("run", list(RUNS))
def test_checkpoint_round_trip_restores_both_nets_and_the_optimiser(g, run):
    weighted = bool(RUNS[run].get("use_priority_weight"))
    a = make_trainer(run)
    a.step(make_sample(0, weighted))
    ckpt = a.get_checkpoint()
    assert list(ckpt["state_dict"]) == [str(k) for k in g["table_fixture_names"]]  # the reference's layout
    b = trainer_api.make(config.Trainer("q-learning", args=RUNS[run]), config.Policy("atari-dqn", args=dict(POLICY, seed=POLICY["seed"] + 1)))
    assert not np.array_equal(state(b)["net.fc.2.weight"], state(a)["net.fc.2.weight"])
    b.load_checkpoint(ckpt)
    sa, sb = state(a), state(b)
    assert all(np.array_equal(sa[k], sb[k]) for k in sa) and b.policy.version == a.policy.version
    oa, ob = a.optimizer.state_dict(), b.optimizer.state_dict()
    assert oa["param_groups"] == ob["param_groups"] and set(oa["state"]) == set(ob["state"])
    for i, st in oa["state"].items():
        assert all(torch.equal(v, ob["state"][i][k]) for k, v in st.items())
    b.steps, b.last_hard_update_step, b.hard_update_count = a.steps, a.last_hard_update_step, a.hard_update_count
    ra, rb = a.step(make_sample(1, weighted)), b.step(make_sample(1, weighted))
    for k in ("value_loss", "grad_norm", "max_td_err"):
        assert ra.stats[k] == rb.stats[k], (k, ra.stats[k], rb.stats[k])
    sa, sb = state(a), state(b)
    assert all(np.array_equal(sa[k], sb[k]) for k in sa)


def test_rollout_through_the_policy(g):
    """Requests through ``rollout``: greedy rows take the argmax of the online Q, epsilon = 1 rows explore, value / target_value are
    the gathers of what ``analyze`` computes for the same frames, with the environment's epsilon and with a scheduler."""
    n = 70
    rng = np.random.default_rng(3)
    frames = rng.integers(0, 256, size=(n, 4, 84, 84), dtype=np.uint8)
    eps = np.where(np.arange(n) % 2 == 0, 0.0, 1.0).astype(np.float32).reshape(n, 1)
    is_eval = (np.arange(n) % 5 == 1).astype(np.uint8).reshape(n, 1)
    policy = policy_api.make(config.Policy("atari-dqn", args=POLICY))
    req = policy_api.RolloutRequest(obs=NamedArray(obs=frames, epsilon=eps), is_evaluation=is_eval,
                                    policy_state=DQNPolicyState(hx=None, epsilon=eps))
    res = policy.rollout(req)
    sample = SampleBatch(obs=NamedArray(obs=frames.reshape(1, n, 4, 84, 84)), on_reset=np.zeros((1, n, 1), np.uint8),
                         action=DiscreteAction(res.action.x.reshape(1, n, 1).astype(np.int32)))
    one = policy_api.make(config.Policy("atari-dqn", args=dict(POLICY, chunk_len=1)))
    out = one.analyze(sample, target="dqn")
    q_on = dqn_ref.dueling_q(out.adv.cpu().numpy(), out.value.cpu().numpy(), np.float32)
    q_tg = dqn_ref.dueling_q(out.target_adv.cpu().numpy(), out.target_value.cpu().numpy(), np.float32)
    greedy, rows, action = q_on.argmax(-1), np.arange(n), res.action.x.reshape(n)
    assert res.action.x.shape == (n, 1) and res.action.x.dtype == np.int64 and ((action >= 0) & (action < ACT)).all()
    exploit = (eps.reshape(n) == 0) | (is_eval.reshape(n) != 0)
    assert np.array_equal(action[exploit], greedy[exploit]) and (action[~exploit] != greedy[~exploit]).any()
    assert close(res.analyzed_result.value.reshape(n), q_on[rows, action], floor=1e-3)
    assert close(res.analyzed_result.target_value.reshape(n), q_tg[rows, greedy], floor=1e-3)
    assert res.analyzed_result.ret is None and res.policy_state.hx is None and np.array_equal(res.policy_state.epsilon, eps)
    again = policy.rollout(req)  # another call: another Philox offset
    assert not np.array_equal(again.action.x, res.action.x)

    class Half:
        def get(self, step):
            return 0.5

    sched = policy_api.make(config.Policy("atari-dqn", args=dict(POLICY, use_env_epsilon=False, epsilon_scheduler=Half())))
    r2 = sched.rollout(policy_api.RolloutRequest(obs=NamedArray(obs=frames), is_evaluation=np.zeros((n, 1), np.uint8)))
    assert (r2.policy_state.epsilon == 0.5).all() and r2.policy_state.epsilon.shape == (n, 1)
    frac = (r2.action.x.reshape(n) != greedy).mean()
    assert 0.1 < frac < 0.8, frac  # about half of the rows explore, five in six of those away from the greedy action
