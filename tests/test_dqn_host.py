"""The Q-learning family without a GPU: registration, the parameter table and the seeded initial weights of ``atari-dqn`` against the
reference's (tests/golden/dqn.npz, written by tests/golden/gen_dqn.py from the real reference), the float64 / float32 restatement
tests/dqn_ref.py pinned against the reference's transforms, ``n_step_return`` and ``DeepQLearning.step`` quantities, the
``n-step-return`` trajectory post-processor, and the sampler's draw."""
import numpy as np
import pytest
import torch

import dqn_ref
import srl_amd
from dqn_cases import POLICY, RUNS, TD_CASES, TD_VARIANTS, assert_within, e2e_arrays, grid, td_case, td_ref
from srl_amd.api import config, policy as policy_api, trainer as trainer_api
from srl_amd.namedarray import NamedArray

srl_amd.register_all()
TABLE_STRIDE = 997


@pytest.fixture(scope="module")
def g(golden):
    return golden("dqn.npz")


def test_registered_under_the_reference_names():
    policy = policy_api.make(config.Policy("atari-dqn", args=POLICY))
    assert policy.default_policy_state.hx is None and policy.default_policy_state.epsilon.shape == (1,)
    trainer = trainer_api.make(config.Trainer("q-learning", args=RUNS["adam"]), config.Policy("atari-dqn", args=POLICY))
    assert trainer.bootstrap_steps == 2 and trainer.optimizer.name == "adam" and trainer.steps == 0
    assert "n-step-return" in trainer_api.ALL_TRAJ_POSTPROCESSOR_CLASSES
    ckpt = trainer.get_checkpoint()
    assert set(ckpt) == {"steps", "state_dict", "optimizer_state_dict"}
    trainer.load_checkpoint(ckpt)


def test_unsupported_options_raise_at_construction():
    mk = lambda **kw: policy_api.make(config.Policy("atari-dqn", args=dict(POLICY, **kw)))
    with pytest.raises(NotImplementedError):
        mk(num_rnn_layers=1)
    with pytest.raises(NotImplementedError):
        mk(dueling=False)
    mkt = lambda **kw: trainer_api.make(config.Trainer("q-learning", args=kw), config.Policy("atari-dqn", args=POLICY))
    with pytest.raises(NotImplementedError):
        mkt(use_popart=True, apply_scalar_transform=False)
    with pytest.raises(ValueError):
        mkt(use_popart=True)
    with pytest.raises(NotImplementedError):
        mkt(mixed_precision=True)
    with pytest.raises(ValueError):
        mkt(bootstrap_steps=0)


@pytest.mark.parametrize("tag,args", [("default", dict(act_dim=18, dueling=True)), ("fixture", POLICY)])
def test_parameter_table_and_seeded_weights_equal_the_reference(g, tag, args):
    sd = policy_api.make(config.Policy("atari-dqn", args=args)).get_checkpoint()["state_dict"]
    assert list(sd) == [str(k) for k in g[f"table_{tag}_names"]]
    assert [tuple(v.shape) for v in sd.values()] == [tuple(int(x) for x in s if x) for s in g[f"table_{tag}_shapes"]]
    samples = np.concatenate([v.numpy().reshape(-1)[::TABLE_STRIDE] for v in sd.values()])
    assert np.array_equal(samples, g[f"table_{tag}_samples"])
    for k, v in sd.items():  # the target is a copy
        if k.startswith("net."):
            assert torch.equal(v, sd["target_" + k])


def test_restated_transforms_and_n_step_return_equal_the_reference(g):
    x = g["prim_x"]
    for eps in (1e-3, 1e-2):
        assert np.array_equal(dqn_ref.scalar_transform(x, eps), g[f"prim_st_{eps}"])
        assert np.array_equal(dqn_ref.inverse_scalar_transform(x, eps), g[f"prim_ist_{eps}"])
    both = 0
    for n in (1, 3, 5):
        pre = f"prim_nstep{n}_"
        ret = dqn_ref.n_step_return(n, g[pre + "reward"], g[pre + "value"], g[pre + "done"], g[pre + "trunc"], 0.97)
        assert ret.dtype == np.float32 and np.array_equal(ret, g[pre + "ret"])
        both += int((g[pre + "done"] * g[pre + "trunc"]).sum())
    assert both > 0  # rows with both flags


@pytest.mark.parametrize("run", list(RUNS))
def test_restated_td_step_equals_the_reference_step(g, run):
    """The reference's analysed q_tot / target_q_tot of the first recorded step through the float32 restatement (one action:
    Q = v, so the gathers are the identity) give its value loss, TD statistics and priorities."""
    targs = RUNS[run]
    arrays = e2e_arrays(0)
    Tb, B = arrays["on_reset"].shape[:2]
    n = Tb * B
    q_tot, target = g[f"{run}_q_tot"].reshape(n), g[f"{run}_target_q_tot"].reshape(n)
    zeros = np.zeros((n, 1), np.float32)
    r = dqn_ref.td_step(zeros, q_tot, zeros, target, np.zeros(n, np.int32), arrays["reward"].reshape(n), arrays["done"].reshape(n),
                        arrays["truncated"].reshape(n), arrays["sampling_weight"] if targs.get("use_priority_weight") else None, Tb, B,
                        n=targs["bootstrap_steps"], gamma=targs.get("gamma", 0.99), value_loss_kind=targs.get("value_loss", "mse"),
                        delta=targs.get("value_loss_config", {}).get("delta", 1.0), dtype=np.float32)
    stats = dict(zip((str(k) for k in g[f"{run}_stat_names"]), g[f"{run}_stats0"]))
    t = r["terms"]
    got = dict(value_loss=t["vloss"] / t["mask"], train_q_tot=t["qinv"] / t["mask"], target_q_tot=t["yinv"] / t["mask"],
               normalized_train_q_tot=t["q"] / t["mask"], normalized_target_q_tot=t["y"] / t["mask"], mean_td_err=t["td"] / t["mask"],
               max_td_err=t["tdmax"], new_priorities=float(r["priorities"].mean()), total_timesteps=t["mask"])
    for k, v in got.items():
        assert abs(v - stats[k]) <= 2e-6 * max(abs(stats[k]), 1e-2), (k, v, stats[k])
    assert np.allclose(r["priorities"], g[f"{run}_priorities0"].reshape(-1), rtol=2e-6, atol=0)
    assert abs(r["loss"] - stats["value_loss"]) <= 2e-6 * abs(stats["value_loss"])


@pytest.mark.parametrize("case", TD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_td_cases_hold_what_they_claim(case):
    """The inputs of the device test: the float32 restatement obeys the rule it sets, and a kernel that broke a tie towards the
    LAST maximum, or dropped the bootstrap-in-advance, would not."""
    c = td_case(*case)
    A = c["A"]
    q_on = dqn_ref.dueling_q(c["adv"], c["v"].reshape(-1, 1), np.float64)
    last = c["B"] - 1
    assert q_on[last].argmax() == 0 and q_on[last][A - 1] == q_on[last][0]  # the tie: first index wins
    assert c["truncated"].reshape(c["T"], c["B"])[c["T"] - 1, last] == 1
    assert (c["done"] & c["truncated"]).any()
    for variant in TD_VARIANTS[:3]:
        r32, r64 = td_ref(c, variant, np.float32), td_ref(c, variant, np.float64)
        for k in ("d_adv", "d_v", "priorities"):
            assert_within(k, r32[k], r32[k], r64[k])
    flipped = dict(c, adv=c["adv"][:, ::-1].copy(), tadv=c["tadv"][:, ::-1].copy(), action=(A - 1 - c["action"]).astype(np.int32))
    a, b = td_ref(c, TD_VARIANTS[0], np.float64), td_ref(flipped, TD_VARIANTS[0], np.float64)
    assert not np.array_equal(a["greedy"][last], A - 1 - b["greedy"][last])  # mirrored actions: the tie resolves the other way


def _memory(reward, tv, tag):
    from srl_amd.algorithm.dqn_policy import DQNRolloutAnalyzedResult
    ep = len(reward)
    mem = []
    for t in range(ep):
        end = np.array([t == ep - 1], dtype=np.uint8)
        mem.append(trainer_api.SampleBatch(obs=NamedArray(obs=np.zeros(1, np.float32)), reward=reward[t], done=end * (tag == "done"),
                                           truncated=end * (tag != "done"),
                                           analyzed_result=DQNRolloutAnalyzedResult(value=tv[t] * 0.5, target_value=tv[t])))
    return mem


@pytest.mark.parametrize("tag,ast", [("done", True), ("trunc", False), ("trunc_st", True)])
def test_n_step_return_postprocessor_equals_the_reference(g, tag, ast):
    pre = f"prim_traj_{tag}_"
    mem = _memory(g[pre + "reward"], g[pre + "target_value"], tag)
    pp = trainer_api.make_traj_postprocessor(config.TrajPostprocessor("n-step-return", args=dict(n=3, gamma=0.9, apply_scalar_transform=ast)))
    pp.process(mem)
    ret = np.stack([np.asarray(m.analyzed_result.ret, np.float64) for m in mem[:-1]])
    want = g[pre + "ret"]
    # float64 sums in another order (the reference filters with scipy); float32 results where the transform rounds
    assert np.allclose(ret, want, rtol=2e-7 if ast else 1e-13, atol=1e-7 if ast else 1e-14), np.abs(ret - want).max()


def test_sampler_draws_are_uniform_over_the_actions():
    """epsilon = 1 over 65 536 rows: every action count within six sigma of n / A (the draw the device test pins bit for bit)."""
    n = 65536
    for A in (6, 18):
        rng = np.random.default_rng(A)
        action, value, _ = dqn_ref.epsilon_greedy_sample(grid(rng, (n, A)), np.zeros(n), grid(rng, (n, A)), np.zeros(n), np.ones(n), None,
                                                         True, seed=3, offset=5, row0=7)
        cnt = np.bincount(action, minlength=A)
        sigma = np.sqrt(n * (1 / A) * (1 - 1 / A))
        assert len(cnt) == A and (np.abs(cnt - n / A) <= 6 * sigma).all(), cnt
