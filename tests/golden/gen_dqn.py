"""Generate tests/golden/dqn.npz: the Q-learning family computed by the REAL reference's own modules (read-only beside this
repository) on the CPU.

Run (from the repo root):
    CUDA_VISIBLE_DEVICES="" PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout>:tests:. python3 tests/golden/gen_dqn.py

Harness-side shims (the reference files stay untouched): a numpy alias and MagicMock for import-time dependencies that are absent.

What it records:
  * ``prim_*``: ``scalar_transform`` / ``inverse_scalar_transform`` (modules/utils.py:324-335) and ``n_step_return``
    (modules/n_step_return.py:11-50) on seeded inputs, and ``TrajNstepReturn`` on a done-terminated and a truncated trajectory;
  * ``table_*``: the parameter table of ``AtariDQNPolicy`` (names, shapes) and strided samples of its seeded initial weights, for
    the default net (hidden_dim 512, seed 42) and the fixture net;
  * ``<run>_*`` for the runs of tests/dqn_cases.py::RUNS: two ``DeepQLearning.step`` calls on the samples of ``e2e_arrays`` -- the
    analyze outputs of the first, statistics and priorities of both, and both networks' parameters after the second as scaled float16
    differences to the initial ones (``packq``; every STRIDE-th element of the two [32, 3136] matrices).
It asserts that in every analysed row the two largest online Q values differ by more than 1e-3 of the row's largest |Q|.
"""
import os
import sys

import numpy as np

np.bool8 = np.bool_
from unittest import mock

for m in ["gym", "gym.spaces", "redis", "redis.backoff", "redis.retry", "wandb", "zmq", "blosc"]:
    sys.modules[m] = mock.MagicMock()
sys.modules.setdefault("mock", mock)
import torch

torch.set_num_threads(1)
import api.config
import api.policy
import api.trainer
from api.env_utils import DiscreteAction
from base.namedarray import NamedArray, recursive_apply
import legacy.algorithm.modules as modules
from legacy.algorithm.modules.n_step_return import TrajNstepReturn, n_step_return
import legacy.algorithm.q_learning.deep_q_learning  # registers "q-learning"
from legacy.algorithm.q_learning.game_policies.atari_dqn_policy import DQNPolicyState, DQNRolloutAnalyzedResult  # registers "atari-dqn"

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from dqn_cases import BIG, POLICY, RUNS, STRIDE, e2e_arrays

TABLE_STRIDE = 997


def packq(out, key, named, before):
    """A state dict as scaled float16 differences to ``before`` (an optimiser step moves a weight by ~5e-4, so eleven bits of the
    difference place it to ~5e-7): ``key_names``, ``key_d`` (float16, the tensors end to end), ``key_e`` per tensor
    (value = before + d 2^-e) and ``key_q`` per tensor: the largest distance of that value to the true one, which the test takes
    OFF its tolerance.  Of the tensors in BIG every STRIDE-th element is kept."""
    names, ds, es, qs = list(named), [], [], []
    for k in names:
        a, b = np.asarray(named[k], np.float64).reshape(-1), np.asarray(before[k], np.float64).reshape(-1)
        if k.split(".", 1)[1] in BIG:
            a, b = a[::STRIDE], b[::STRIDE]
        d = a - b
        top = float(np.abs(d).max())
        e = int(9 - np.floor(np.log2(top))) if top > 0 else 0
        d16 = (d * 2.0**e).astype(np.float16)
        ds.append(d16)
        es.append(e)
        qs.append(np.abs(b + d16.astype(np.float64) * 2.0**-e - a).max())
    out[key + "_names"], out[key + "_d"], out[key + "_e"], out[key + "_q"] = np.array(names), np.concatenate(ds), np.array(es), np.array(qs)
    return max(qs)


def gen_primitives(out):
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.standard_normal(40) * 10.0 ** rng.integers(-3, 4, size=40), [0.0, -0.0, 1e-8, -300.0]]).astype(np.float32)
    out["prim_x"] = x
    for eps in (1e-3, 1e-2):
        out[f"prim_st_{eps}"] = modules.scalar_transform(torch.from_numpy(x), eps=eps).numpy()
        out[f"prim_ist_{eps}"] = modules.inverse_scalar_transform(torch.from_numpy(x), eps=eps).numpy()
    for n, T, B in ((1, 4, 3), (3, 7, 5), (5, 2, 4)):
        L = n + T - 1
        reward, value = rng.standard_normal((L, B, 1)).astype(np.float32), rng.standard_normal((L, B, 1)).astype(np.float32)
        done = (rng.random((L, B, 1)) < 0.2).astype(np.float32)
        trunc = (rng.random((L, B, 1)) < 0.2).astype(np.float32)   # some rows carry both flags
        ret = n_step_return(n, *map(torch.from_numpy, (reward, value, done, trunc)), gamma=0.97)
        pre = f"prim_nstep{n}_"
        out[pre + "reward"], out[pre + "value"], out[pre + "done"], out[pre + "trunc"], out[pre + "ret"] = reward, value, done, trunc, ret.numpy()
    for tag, ast in (("done", True), ("trunc", False), ("trunc_st", True)):
        ep, n = 9, 3
        reward = rng.standard_normal((ep, 1)).astype(np.float32)
        tv = rng.standard_normal((ep, 1)).astype(np.float32)
        memory = []
        for t in range(ep):
            end = np.array([t == ep - 1], dtype=np.uint8)
            memory.append(api.trainer.SampleBatch(obs=NamedArray(obs=np.zeros(1, np.float32)), reward=reward[t],
                                                  done=end * (tag == "done"), truncated=end * (tag != "done"),
                                                  analyzed_result=DQNRolloutAnalyzedResult(value=tv[t] * 0.5, target_value=tv[t])))
        TrajNstepReturn(n=n, gamma=0.9, apply_scalar_transform=ast).process(memory)
        pre = f"prim_traj_{tag}_"
        out[pre + "reward"], out[pre + "target_value"] = reward, tv
        out[pre + "ret"] = np.stack([np.asarray(m.analyzed_result.ret, np.float64) for m in memory[:-1]])


def gen_table(out, tag, **args):
    policy = api.policy.make(api.config.Policy("atari-dqn", args=args))
    sd = policy.net.state_dict()
    out[f"table_{tag}_names"] = np.array(list(sd))
    out[f"table_{tag}_shapes"] = np.array([tuple(v.shape) + (0,) * (4 - v.dim()) for v in sd.values()])
    out[f"table_{tag}_samples"] = np.concatenate([v.numpy().reshape(-1)[::TABLE_STRIDE] for v in sd.values()])
    out[f"table_{tag}_optim_params"] = np.array(len(list(policy.parameters())))


def ref_sample(arrays, weighted):
    Tb, B = arrays["on_reset"].shape[:2]
    return api.trainer.SampleBatch(obs=NamedArray(obs=arrays["obs.obs"]),
                                   policy_state=DQNPolicyState(hx=None, epsilon=arrays["policy_state.epsilon"]),
                                   on_reset=arrays["on_reset"], done=arrays["done"], truncated=arrays["truncated"],
                                   action=DiscreteAction(arrays["action.x"]), reward=arrays["reward"],
                                   info_mask=arrays["info_mask"], sampling_weight=arrays["sampling_weight"] if weighted else None)


def sd_np(net):
    return {k: v.detach().cpu().numpy().copy() for k, v in net.state_dict().items()}


def gen_run(out, run, targs):
    trainer = api.trainer.make(api.config.Trainer("q-learning", args=targs), api.config.Policy("atari-dqn", args=POLICY))
    policy = trainer.policy
    init = sd_np(policy.net)
    weighted = bool(targs.get("use_priority_weight"))
    for step in range(2):
        arrays = e2e_arrays(step)
        sample = ref_sample({k: v.copy() for k, v in arrays.items()}, weighted)
        if not weighted:
            sample.pop_metadata("sampling_weight")
        ts = recursive_apply(sample, lambda x: torch.from_numpy(x).to(torch.float32))
        with torch.no_grad():
            ar = policy.analyze(ts, burn_in_steps=0)
            qf, _ = policy.net(ts.obs.obs / 255., None, ts.on_reset)
        top2 = torch.topk(qf, 2, dim=-1).values
        gap = ((top2[..., 0] - top2[..., 1]) / qf.abs().max(-1).values).min().item()
        assert gap > 1e-3, f"{run} step {step}: near-tie of the two largest online Q values ({gap:.2e}); choose another seed"
        if step == 0:
            out[f"{run}_q_tot"], out[f"{run}_target_q_tot"] = ar.q_tot.numpy(), ar.target_q_tot.numpy()
        before_target = {k: v for k, v in sd_np(policy.net).items() if k.startswith("target_net.")}
        res = trainer.step(sample)
        stats = {k: float(v) for k, v in res.stats.items()}
        out[f"{run}_stat_names"] = np.array(sorted(stats))
        out[f"{run}_stats{step}"] = np.array([stats[k] for k in sorted(stats)], dtype=np.float64)
        out[f"{run}_priorities{step}"] = np.asarray(res.priorities)
        out[f"{run}_step{step}"] = np.array(res.step)
        after = sd_np(policy.net)
        moved = any(not np.array_equal(after[k], v) for k, v in before_target.items())
        out[f"{run}_target_moved{step}"] = np.array(moved)
        print(f"{run} step {step}: smallest relative Q gap {gap:.2e}, target moved {moved}, value_loss {stats['value_loss']:.6f}")
    q = packq(out, f"{run}_final", after, init)
    print(f"{run}: the encoding places the parameters to {q:.2e}")
    out[f"{run}_optim_state_params"] = np.array(len(trainer.optimizer.state_dict()["state"]))


if __name__ == "__main__":
    out = {}
    gen_primitives(out)
    gen_table(out, "default", act_dim=18, dueling=True)
    gen_table(out, "fixture", **POLICY)
    for run, targs in RUNS.items():
        gen_run(out, run, targs)
    out["torch_version"] = np.array(torch.__version__)
    path = os.path.join(HERE, "dqn.npz")
    np.savez_compressed(path, **out)
    print(f"wrote dqn.npz: {os.path.getsize(path)} bytes, {len(out)} arrays")
    assert os.path.getsize(path) < 1_000_000
