"""Generate tests/golden/r2d2.npz: the recurrent ``atari-dqn`` agent (R2D2) computed by the REAL reference's own modules (read-only
beside this repository) on the CPU.

Run (from the repo root):
    CUDA_VISIBLE_DEVICES="" PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout>:tests:. python3 tests/golden/gen_r2d2.py

Harness-side shims (the reference files stay untouched): a numpy alias and MagicMock for import-time dependencies that are absent.

What it records (cases: tests/r2d2_cases.py):
  * ``table_*``: the parameter table of ``AtariDQNPolicy`` (names, shapes) and strided samples of its seeded initial weights for
    GRU x 1 layer and LSTM x 2 layers at hidden_dim 512;
  * ``<run>_*`` for the runs ``gru`` (burn-in) and ``lstm``: two ``DeepQLearning.step`` calls -- the analyze outputs of the first,
    statistics and priorities of both, and both networks' parameters after the second as scaled float16 differences to the initial
    ones (``packq``; every ``r2d2_cases.stride_of``-th element of each tensor);
  * ``<run>_f64_<quantity>``: the same run with the networks and the sample in float64, and per compared quantity the largest
    distance of the float32 run from it in units of the bar the tests hold that quantity to.
It asserts that ``on_reset`` is set inside chunks and (with burn-in) inside a burn-in window, and that in every analysed row the two
largest online Q values differ by more than 1e-3 of the row's largest |Q|.
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
import legacy.algorithm.q_learning.deep_q_learning as dql  # registers "q-learning"
from legacy.algorithm.q_learning.game_policies.atari_dqn_policy import DQNPolicyState  # registers "atari-dqn"

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from r2d2_cases import PARAM_TOL, RUNS, TABLES, TABLE_STRIDE, e2e_arrays, rel_err, stride_of


TENSOR_FLOAT = torch.Tensor.float


def packq(out, key, named, before):
    """A state dict as scaled float16 differences to ``before`` (gen_dqn.packq), every ``stride_of(numel)``-th element of each
    tensor: ``key_names``, ``key_d``, ``key_e`` per tensor (value = before + d 2^-e) and ``key_q`` per tensor, the largest distance
    of that value to the true one, which the test takes OFF its tolerance."""
    names, ds, es, qs = list(named), [], [], []
    for k in names:
        a, b = np.asarray(named[k], np.float64).reshape(-1), np.asarray(before[k], np.float64).reshape(-1)
        s = stride_of(a.size)
        a, b = a[::s], b[::s]
        d = a - b
        top = float(np.abs(d).max())
        e = int(9 - np.floor(np.log2(top))) if top > 0 else 0
        d16 = (d * 2.0**e).astype(np.float16)
        ds.append(d16)
        es.append(e)
        qs.append(np.abs(b + d16.astype(np.float64) * 2.0**-e - a).max())
    out[key + "_names"], out[key + "_d"], out[key + "_e"], out[key + "_q"] = np.array(names), np.concatenate(ds), np.array(es), np.array(qs)
    return max(qs)


def gen_table(out, tag, args):
    policy = api.policy.make(api.config.Policy("atari-dqn", args=args))
    sd = policy.net.state_dict()
    out[f"table_{tag}_names"] = np.array(list(sd))
    out[f"table_{tag}_shapes"] = np.array([tuple(v.shape) + (0,) * (4 - v.dim()) for v in sd.values()])
    out[f"table_{tag}_samples"] = np.concatenate([v.numpy().reshape(-1)[::TABLE_STRIDE] for v in sd.values()])
    hx = policy.default_policy_state.hx
    out[f"table_{tag}_default_hx_shape"] = np.array(hx.shape)
    assert not hx.any() and hx.dtype == np.float32


def ref_sample(arrays, weighted):
    return api.trainer.SampleBatch(obs=NamedArray(obs=arrays["obs.obs"]),
                                   policy_state=DQNPolicyState(hx=arrays["policy_state.hx"], epsilon=arrays["policy_state.epsilon"]),
                                   on_reset=arrays["on_reset"], done=arrays["done"], truncated=arrays["truncated"],
                                   action=DiscreteAction(arrays["action.x"]), reward=arrays["reward"],
                                   info_mask=arrays["info_mask"], sampling_weight=arrays["sampling_weight"] if weighted else None)


def sd_np(net):
    return {k: v.detach().cpu().numpy().copy() for k, v in net.state_dict().items()}


def check_resets(run, step, arrays):
    r = RUNS[run]
    burn, cl = r["trainer"].get("burn_in_steps", 0), r["policy"]["chunk_len"]
    rs = arrays["on_reset"][..., 0]
    T = rs.shape[0] - burn
    K = T // cl
    C = T // K
    inside = np.ones(T, bool)
    inside[::C] = False   # not a chunk's first step
    assert rs[burn:][inside].any(), f"{run} step {step}: no on_reset inside a chunk; choose another sample seed"
    if burn:
        win = np.zeros(rs.shape[0], bool)
        for k in range(K):
            win[k * cl + 1:k * cl + burn] = True   # behind the window's first row
        assert rs[win].any(), f"{run} step {step}: no on_reset inside a burn-in window; choose another sample seed"


def run_steps(run, dtype):
    r = RUNS[run]
    targs = r["trainer"]
    burn = targs.get("burn_in_steps", 0)
    trainer = api.trainer.make(api.config.Trainer("q-learning", args=targs), api.config.Policy("atari-dqn", args=r["policy"]))
    policy = trainer.policy
    init = sd_np(policy.net)
    if dtype == torch.float64:   # the networks and the whole sample in float64 (``step`` converts its sample to float32 itself:
        # its module's ``recursive_apply`` and ``Tensor.float`` are shimmed for the length of this run)
        policy.net.double()
        dql.recursive_apply = lambda s, fn: recursive_apply(s, lambda x: torch.from_numpy(x).to(torch.float64))
        torch.Tensor.float = lambda self: self   # (the transforms and the n-step return round their float64 results: not in this run)
    weighted = bool(targs.get("use_priority_weight"))
    online = []
    policy.net.net.register_forward_hook(lambda mod, args, output: online.append(output[0].detach()))
    rec = {}
    for step in range(2):
        arrays = e2e_arrays(run, step)
        check_resets(run, step, arrays)
        sample = ref_sample({k: v.copy() for k, v in arrays.items()}, weighted)
        if not weighted:
            sample.pop_metadata("sampling_weight")
        ts = recursive_apply(sample, lambda x: torch.from_numpy(x).to(dtype))
        del online[:]
        with torch.no_grad():
            ar = policy.analyze(ts, burn_in_steps=burn)
        qf = online[-1]   # the online network's main pass (a burn-in pass comes before it)
        top2 = torch.topk(qf, 2, dim=-1).values
        gap = ((top2[..., 0] - top2[..., 1]) / qf.abs().max(-1).values).min().item()
        assert gap > 1e-3, f"{run} step {step}: near-tie of the two largest online Q values ({gap:.2e}); choose another seed"
        if step == 0:
            rec["q_tot"], rec["target_q_tot"] = ar.q_tot.numpy(), ar.target_q_tot.numpy()
        before_target = {k: v for k, v in sd_np(policy.net).items() if k.startswith("target_net.")}
        res = trainer.step(sample)
        stats = {k: float(v) for k, v in res.stats.items()}
        rec["stat_names"] = np.array(sorted(stats))
        rec[f"stats{step}"] = np.array([stats[k] for k in sorted(stats)], dtype=np.float64)
        rec[f"priorities{step}"] = np.asarray(res.priorities)
        rec[f"step{step}"] = np.array(res.step)
        after = sd_np(policy.net)
        rec[f"target_moved{step}"] = np.array(any(not np.array_equal(after[k], v) for k, v in before_target.items()))
        print(f"{run} {dtype} step {step}: smallest relative Q gap {gap:.2e}, value_loss {stats['value_loss']:.6f}")
    rec["optim_state_params"] = np.array(len(trainer.optimizer.state_dict()["state"]))
    dql.recursive_apply = recursive_apply
    torch.Tensor.float = TENSOR_FLOAT
    return rec, init, after


def gen_run(out, run):
    r32, init, after32 = run_steps(run, torch.float32)
    r64, _, after64 = run_steps(run, torch.float64)
    for k, v in r32.items():
        out[f"{run}_{k}"] = v
    q = packq(out, f"{run}_final", after32, init)
    print(f"{run}: the encoding places the parameters to {q:.2e}")
    # the reference's own float32 run against its float64 run, in units of each quantity's bar
    dist = dict(q_tot=rel_err(r32["q_tot"], r64["q_tot"], 1e-3) / 1e-5, target_q_tot=rel_err(r32["target_q_tot"], r64["target_q_tot"], 1e-3) / 1e-5,
                params=max(float(np.abs(after32[k].astype(np.float64) - after64[k]).max()) for k in after32) / PARAM_TOL)
    for step in range(2):
        dist[f"stats{step}"] = rel_err(r32[f"stats{step}"], r64[f"stats{step}"], 1e-2) / 1e-5
        dist[f"priorities{step}"] = rel_err(r32[f"priorities{step}"], r64[f"priorities{step}"], 1e-3) / 1e-5
    for k, v in dist.items():
        out[f"{run}_f64_{k}"] = np.array(v)
        print(f"{run}: float32 to float64, {k}: {v:.3f} of the bar")


if __name__ == "__main__":
    out = {}
    for tag, args in TABLES.items():
        gen_table(out, tag, args)
    for run in RUNS:
        gen_run(out, run)
    out["torch_version"] = np.array(torch.__version__)
    path = os.path.join(HERE, "r2d2.npz")
    np.savez_compressed(path, **out)
    print(f"wrote r2d2.npz: {os.path.getsize(path)} bytes, {len(out)} arrays")
    assert os.path.getsize(path) < 1_000_000
