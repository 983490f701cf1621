"""Generate tests/golden/steps_smac_attn.npz: the agent-specific (attention) encoders of ``smac_rnn`` computed by the REAL
reference's own modules (read-only beside this repository), once in float32 and once in float64.

Run (from the repo root):
    CUDA_VISIBLE_DEVICES="" PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout>:. python3 tests/golden/gen_smac_attn.py

Harness-side shims (the reference files stay untouched), beside those of gen_golden.py (numpy alias, MagicMock for absent
import-time dependencies, a CPU pass-through for the CUDA prefetcher):

1. head count: ``SMACAgentwiseEncoder`` (smac_rnn.py:35) calls ``MultiHeadSelfAttention(H/2, H/2, 4)`` where the signature is
   ``(input_dim, heads, d_head)`` (attention.py:62): H/2 heads of width 4, a 2H-wide output, and ``LayerNorm(H)`` raises on the
   2.5H-wide concatenation.  While a policy / encoder is built, ``modules.MultiHeadSelfAttention`` is replaced by
   ``lambda i, d, h: Orig(i, h, d // h)``: input H/2, 4 heads of H/8 -- the order hns_policy.py:49 uses.
2. ``legacy.environment.smac.smac_env`` needs StarCraft: a stand-in supplies ``SMACAction`` and ``get_smac_shapes``.
3. rollout only: the reference's default state is H wide where its LSTM needs 2H (gen_golden.py gen_smac, shim 3).
4. float64 run only: the network is cast with ``.double()`` after construction (same initial values), and the reference's
   explicit casts to float32 (``.float()`` in gae.py:97 and utils.py:67,144,151; ``dtype=torch.float32`` in the rollout,
   smac_rnn.py:346-347) are made to keep float64.

Float64 quantities are stored as scaled float16 differences to the float32 run (``put64``), which halves the file.
"""
import copy
import os
import sys
import types

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

DTYPE = [torch.float32]


class CPUPrefetcher:

    def push(self, sample):
        return sample, recursive_apply(sample, lambda x: torch.from_numpy(x).to(DTYPE[0]))


api.trainer.PyTorchGPUPrefetcher = CPUPrefetcher
import legacy.algorithm.ppo.mappo as mappo

mappo.PyTorchGPUPrefetcher = CPUPrefetcher
import legacy.algorithm.modules as modules
from legacy.algorithm.ppo.actor_critic_policies.actor_critic_policy import PPORolloutAnalyzedResult

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from srl_amd.runtime import synthetic

SHAPES = [None]
fake = types.ModuleType("legacy.environment.smac.smac_env")


class SMACAction(DiscreteAction):
    pass


fake.SMACAction = SMACAction
fake.get_smac_shapes = lambda map_name, **kw: SHAPES[0]
sys.modules["legacy.environment.smac.smac_env"] = fake
import legacy.algorithm.ppo.game_policies.smac_rnn as smac_rnn  # registers "smac_rnn"

_OrigMHSA = modules.MultiHeadSelfAttention


class head_count_shim:

    def __enter__(self):
        modules.MultiHeadSelfAttention = lambda i, d, h: _OrigMHSA(i, h, d // h)

    def __exit__(self, *exc):
        modules.MultiHeadSelfAttention = _OrigMHSA


def put64(out, key, v64, v32):
    """out[key + "64d"] (float16) and out[key + "64e"] (k): value64 = float64(value32) + float64(d) * 2 ** -k.  The difference is
    the float32 run's own rounding error; eleven bits of it place the float64 value to ~1e-10 of the tensor's scale."""
    d = np.asarray(v64, np.float64) - np.asarray(v32, np.float64)
    top = float(np.abs(d).max()) if d.size else 0.0
    k = int(9 - np.floor(np.log2(top))) if top > 0 else 0
    out[key + "64d"], out[key + "64e"] = (d * 2.0**k).astype(np.float16), np.array(k)


def pack(out, key, named, named64=None):
    """A name -> array dict as a few arrays (an .npz entry costs ~200 bytes of headers; a state dict has 79): ``key_names``,
    ``key_shapes`` ([tensors, 2], columns 0 for vectors) and ``key_flat`` for the float32 tensors, ``key_f64:<name>`` for the float64
    ones (PopArt's running statistics); with ``named64`` the float64 run's values as ``key_flat64d`` / ``key_flat64e`` (``put64``
    per tensor, exponents side by side).  tests/smac_attn_cases.py has the inverse."""
    names = [k for k, v in named.items() if v.dtype != np.float64]
    out[key + "_names"] = np.array(names)
    out[key + "_shapes"] = np.array([(v.shape[0], v.shape[1] if v.ndim > 1 else 0) for v in (named[k] for k in names)])
    out[key + "_flat"] = np.concatenate([named[k].reshape(-1) for k in names]).astype(np.float32)
    for k, v in named.items():
        if v.dtype == np.float64:
            out[f"{key}_f64:{k}"] = v
    if named64 is not None:
        ds, es, tmp = [], [], {}
        for k in names:
            put64(tmp, "x", named64[k], named[k])
            ds.append(tmp["x64d"].reshape(-1))
            es.append(int(tmp["x64e"]))
        out[key + "_flat64d"], out[key + "_flat64e"] = np.concatenate(ds), np.array(es)


# ------------------------------------------------------------------------------------------------ block cases
CASES = {  # name: (D, S, [(leaf, entities, features)], rows)
    "a": (16, 7, [("allies", 2, 5), ("enemies", 3, 6), ("move", 1, 4)], 37),
    "b": (32, 20, [("allies", 4, 5), ("enemies", 4, 6), ("move", 1, 4)], 130),
    "c": (16, 9, [("allies", 3, 8), ("enemies", 3, 7)], 5),
    "d": (64, 40, [("allies", 31, 4), ("enemies", 32, 4), ("move", 1, 4)], 3),
}


def gen_block(name, out):
    D, S, keys, n = CASES[name]
    E = sum(c for _, c, _ in keys)
    rng = np.random.default_rng(1000 + ord(name))
    shapes = {"obs_self": (S,), "obs_mask": (E,), **{f"obs_{k}": (c, f) for k, c, f in keys}}
    with head_count_shim():
        enc = smac_rnn.SMACAgentwiseObsEncoder(shapes, 2 * D)
    # seeded parameters on a coarse grid (multiples of 1/64: exact in float32, and the file compresses); LayerNorm weights around 1
    with torch.no_grad():
        for k, p in enc.named_parameters():
            g = rng.integers(-24, 25, size=tuple(p.shape)).astype(np.float32) / 64.0
            if "norm" in k and k.endswith("weight"):
                g = 1.0 + g / 2
            elif p.dim() == 2:
                g = g * 2.0**np.round(np.log2(3.0 / np.sqrt(p.shape[1])))  # (a power of two: the grid stays exact)
            p.copy_(torch.from_numpy(g.astype(np.float32)))
    x = {"obs_self": rng.integers(-64, 65, size=(n, S)).astype(np.float32) / 32.0}
    for k, c, f in keys:
        x[f"obs_{k}"] = rng.integers(-64, 65, size=(n, c, f)).astype(np.float32) / 32.0
    mask = (rng.random((n, E)) < 0.7).astype(np.uint8)
    if name == "a":  # rows without any entity, with one, with all
        mask[0], mask[1], mask[2] = 0, 0, 1
        mask[1, 3] = 1
        mask[36] = 0
    if name == "d":
        mask[0] = 1
        mask[2] = 0
        mask[2, 63] = 1
    cot = rng.integers(-64, 65, size=(n, 2 * D)).astype(np.float32) / 64.0
    res = {}
    for tag, dt in (("32", torch.float32), ("64", torch.float64)):
        e = copy.deepcopy(enc).to(dt)
        got = []
        e.encoder.dense.register_forward_pre_hook(lambda mod, inp: got.append(inp[0]))  # cat(self_emb, pooled) (smac_rnn.py:43)
        obs = NamedArray(obs_mask=torch.from_numpy(mask).to(dt), **{k: torch.from_numpy(v).to(dt) for k, v in x.items()})
        e(obs)
        (got[0] * torch.from_numpy(cot).to(dt)).sum().backward()
        res[tag] = (got[0].detach().numpy(), {k: p.grad.numpy() for k, p in e.named_parameters() if not k.startswith("encoder.dense")})
    pre = f"blk_{name}_"
    out[pre + "dims"] = np.array([D, S, n, E])
    out[pre + "keys"] = np.array([f"obs_{k}" for k, _, _ in keys])
    out[pre + "mask"], out[pre + "cot"] = mask, cot
    for k, v in x.items():
        out[pre + "x." + k] = v
    pack(out, pre + "param", {k: p.detach().numpy() for k, p in enc.named_parameters() if not k.startswith("encoder.dense")})
    out[pre + "out32"] = res["32"][0]
    put64(out, pre + "out", res["64"][0], res["32"][0])
    pack(out, pre + "grad", res["32"][1], res["64"][1])
    err = max(np.abs(res["64"][1][k] - res["32"][1][k]).max() / max(np.abs(res["64"][1][k]).max(), 1e-30) for k in res["32"][1]
              if "k_linear.bias" not in k)
    print(f"block {name}: rows {n} E {E} all-masked rows {(mask.sum(1) == 0).sum()}, float32 gradient error (rel. to max) {err:.2e}, "
          f"k_linear.bias {np.abs(res['64'][1]['encoder.attn.k_linear.bias']).max():.1e} / "
          f"q_linear.bias {np.abs(res['64'][1]['encoder.attn.q_linear.bias']).max():.1e}")


# ------------------------------------------------------------------------------------------------ trainer run
H, A, CL, ACT = 32, 3, 5, 9
OBS = {"obs_allies": (2, 5), "obs_enemies": (3, 6), "obs_move": (1, 4), "obs_self": (7,), "obs_mask": (6,)}
STATE = {"state_allies": (2, 8), "state_enemies": (3, 7), "state_move": (1, 4), "state_self": (9,), "state_mask": (6,)}
TRAINER = dict(popart=True, ppo_epochs=2, optimizer_config=dict(lr=5e-4, eps=1e-5), max_grad_norm=10.0,
               value_loss="huber", value_loss_config=dict(delta=10.0), clip_value=True, dual_clip=False)
SAMPLE = dict(T=10, B=2, agents=A, obs_spec={"local_obs": ((1,), "f32")}, action_dim=ACT, p_done=0.08,
              policy_state={"actor_hx": (1, 2 * H), "critic_hx": (1, 2 * H)})


def nested(rng, lead, shapes):
    out = {}
    for k, shp in shapes.items():
        if k.endswith("_mask"):
            m = (rng.random((*lead, *shp)) < 0.75).astype(np.float32)
            m[..., 0] = np.where(rng.random(lead) < 0.9, 1.0, m[..., 0])
            out[k] = m
        else:
            out[k] = rng.standard_normal((*lead, *shp)).astype(np.float32)
    return out


def make_arrays(seed):
    arrays = synthetic.make_multiagent_arrays(seed=seed, **SAMPLE)
    arrays.pop("obs.local_obs")
    rng = np.random.default_rng(seed + 77)
    lead = arrays["on_reset"].shape[:3]
    for k, v in nested(rng, lead, OBS).items():
        arrays[f"obs.local_obs.{k}"] = v
    for k, v in nested(rng, lead, STATE).items():
        arrays[f"obs.state.{k}"] = v
    return arrays


def obs_tree(arrays, state_flat=None):
    loc = NamedArray(**{k[len("obs.local_obs."):]: v for k, v in arrays.items() if k.startswith("obs.local_obs.")})
    st = state_flat if state_flat is not None else NamedArray(**{k[len("obs.state."):]: v for k, v in arrays.items()
                                                                 if k.startswith("obs.state.")})
    return NamedArray(local_obs=loc, state=st, available_action=arrays["obs.available_action"], is_alive=arrays["obs.is_alive"])


def ref_sample(arrays, state_flat=None):
    return api.trainer.SampleBatch(obs=obs_tree(arrays, state_flat),
                                   policy_state=NamedArray(actor_hx=arrays["policy_state.actor_hx"],
                                                           critic_hx=arrays["policy_state.critic_hx"]),
                                   on_reset=arrays["on_reset"], done=arrays["done"], truncated=arrays["truncated"],
                                   action=DiscreteAction(arrays["action.x"]), reward=arrays["reward"],
                                   analyzed_result=PPORolloutAnalyzedResult(log_probs=arrays["analyzed_result.log_probs"],
                                                                            value=arrays["analyzed_result.value"]),
                                   policy_version_steps=arrays["policy_version_steps"], info_mask=arrays["info_mask"])


def make_trainer(obs_shape, state_shape, aso, ass, dt):
    SHAPES[0] = (obs_shape, state_shape, ACT, A)
    pargs = dict(map_name="3m", hidden_dim=H, chunk_len=CL, seed=31, shared=True, agent_specific_obs=aso, agent_specific_state=ass)
    with head_count_shim():
        trainer = api.trainer.make(api.config.Trainer("mappo", args=TRAINER), api.config.Policy("smac_rnn", args=pargs))
    if dt == torch.float64:
        trainer.policy.net.double()  # the float32 initial values, exactly; the optimiser keeps the same Parameter objects
    return trainer


def sd_np(net):
    return {k: v.detach().cpu().numpy().copy() for k, v in net.state_dict().items()}


def run_trainer(dt):
    DTYPE[0] = dt
    r = {}
    trainer = make_trainer(OBS, STATE, True, True, dt)
    net = trainer.policy.net
    r["init"] = sd_np(net)
    for step in range(2):
        arrays = make_arrays(400 + step)
        r[f"sample{step}"] = {k: v for k, v in arrays.items() if k.startswith(("obs.local_obs.", "obs.state."))}
        sample = ref_sample({k: v.copy() for k, v in arrays.items()})
        if step == 0:
            ts = recursive_apply(sample, lambda x: torch.from_numpy(x).to(dt))
            Tb = arrays["on_reset"].shape[0]
            with torch.no_grad():
                ar = trainer.policy.analyze(ts[:Tb - 1], target="ppo", burn_in_steps=0)
            r["analyze"] = (ar.new_action_log_probs.numpy(), ar.state_values.numpy(), ar.entropy.numpy())
        res = trainer.step(sample)
        stats = {k: float(v) for k, v in res.stats.items()}
        r["stat_names"] = sorted(stats)
        r[f"stats{step}"] = np.array([stats[k] for k in r["stat_names"]], dtype=np.float64)
        if step == 0:
            r["adv"], r["ret"] = np.asarray(sample.analyzed_result.adv), np.asarray(sample.analyzed_result.ret)
        r[f"param{step}"] = sd_np(net)
    r["version"] = trainer.policy.version
    # deterministic rollout on [N, agents, ...] requests with the trained weights
    policy = trainer.policy
    setattr(policy, "_SMACPolicy__rnn_default_hidden", np.zeros((A, 1, 2 * H), dtype=np.float32))  # shim 3
    rng = np.random.default_rng(12)
    N = 5
    avail = (rng.random((N, A, ACT)) < 0.6).astype(np.uint8)
    avail[..., 0] = 1
    req = {}
    for k, v in nested(rng, (N, A), OBS).items():
        req[f"local_obs.{k}"] = v
    for k, v in nested(rng, (N, A), STATE).items():
        req[f"state.{k}"] = v
    hx = (0.5 * rng.standard_normal((2, N, A, 1, 2 * H))).astype(np.float32)
    on_reset = (rng.random((N, 1, 1)) < 0.4).astype(np.uint8).repeat(A, axis=1)
    aux = {k: np.zeros((N, A), dtype=np.int32) for k in ("client_id", "request_id", "received_time", "buffer_index",
                                                          "step_count", "ready")}
    obs = NamedArray(local_obs=NamedArray(**{k[len("local_obs."):]: v for k, v in req.items() if k.startswith("local_obs.")}),
                     state=NamedArray(**{k[len("state."):]: v for k, v in req.items() if k.startswith("state.")}),
                     available_action=avail, is_alive=np.ones((N, A, 1), dtype=np.uint8))
    rr = api.policy.RolloutRequest(obs=obs, policy_state=NamedArray(actor_hx=hx[0], critic_hx=hx[1]),
                                   is_evaluation=np.ones((N, A, 1), dtype=np.uint8), on_reset=on_reset, **aux)
    if dt == torch.float64:  # the reference's rollout casts its requests to float32 (smac_rnn.py:346-347): keep the float64 net
        orig = torch.Tensor.to
        with mock.patch.object(torch.Tensor, "to", lambda self, *a, **k: orig(self, *a, **{**k, "dtype": dt}) if k.get("dtype") == torch.float32 else orig(self, *a, **k)):
            res = policy.rollout(rr)
    else:
        res = policy.rollout(rr)
    r["roll_in"] = dict(req, available_action=avail, actor_hx=hx[0], critic_hx=hx[1], on_reset=on_reset)
    r["roll"] = dict(action=res.action.x, log_probs=res.analyzed_result.log_probs, value=res.analyzed_result.value,
                     new_actor_hx=res.policy_state.actor_hx, new_critic_hx=res.policy_state.critic_hx)
    return r


def gen_trainer(out):
    r32 = run_trainer(torch.float32)
    # float64 run: the reference casts to float32 at a few places (gae.py:97, utils.py:67,144,151); `.float()` keeps float64 here
    with mock.patch.object(torch.Tensor, "float", lambda self: self.double()):
        r64 = run_trainer(torch.float64)
    pack(out, "init", r32["init"])
    for k, v in r32["init"].items():
        assert np.array_equal(np.asarray(r64["init"][k], np.float64), np.asarray(v, np.float64)), k
    print(f"state dict: {len(r32['init'])} tensors, {sum(v.size for v in r32['init'].values())} values")
    out["stat_names"], out["version"] = np.array(r32["stat_names"]), np.array(r32["version"])
    for i, name in enumerate(("new_lp", "value", "entropy")):
        out[f"analyze_{name}"] = r32["analyze"][i]
        a64 = np.where(np.isfinite(r64["analyze"][i]), r64["analyze"][i], 0.0)
        a32 = np.where(np.isfinite(r32["analyze"][i]), r32["analyze"][i], 0.0)
        put64(out, f"analyze_{name}", a64, a32)
    out["step0_adv"], out["step0_ret"] = r32["adv"], r32["ret"]
    put64(out, "step0_adv", r64["adv"], r32["adv"])
    put64(out, "step0_ret", r64["ret"], r32["ret"])
    for step in range(2):
        for k, v in r32[f"sample{step}"].items():  # the nested observation leaves; the flat leaves are synthetic.make_multiagent_arrays'
            out[f"sample{step}.{k}"] = v
        out[f"step{step}_stats"], out[f"step{step}_stats64"] = r32[f"stats{step}"], r64[f"stats{step}"]
        pack(out, f"step{step}", r32[f"param{step}"], r64[f"param{step}"])
    for k, v in r32["roll_in"].items():
        out[f"roll_in.{k}"] = v
    for k, v in r32["roll"].items():
        out[f"roll_{k}"] = np.asarray(v)
        if k != "action":
            put64(out, f"roll_{k}", r64["roll"][k], v)
    assert np.array_equal(r32["roll"]["action"], r64["roll"]["action"])
    # one mixed policy: attention on the observation side, a flat state
    DTYPE[0] = torch.float32
    trainer = make_trainer(OBS, (11,), True, False, torch.float32)
    arrays = make_arrays(400)
    state_flat = np.random.default_rng(5).standard_normal((*arrays["on_reset"].shape[:3], 11)).astype(np.float32)
    ts = recursive_apply(ref_sample(arrays, state_flat), lambda x: torch.from_numpy(x).float())
    Tb = arrays["on_reset"].shape[0]
    with torch.no_grad():
        ar = trainer.policy.analyze(ts[:Tb - 1], target="ppo", burn_in_steps=0)
    out["mixed_state"] = state_flat
    out["mixed_new_lp"], out["mixed_value"], out["mixed_entropy"] = (ar.new_action_log_probs.numpy(), ar.state_values.numpy(),
                                                                     ar.entropy.numpy())
    pack(out, "mixed_init", sd_np(trainer.policy.net))


if __name__ == "__main__":
    out = {}
    for name in CASES:
        gen_block(name, out)
    gen_trainer(out)
    out["torch_version"] = np.array(torch.__version__)
    path = os.path.join(HERE, "steps_smac_attn.npz")
    np.savez_compressed(path, **out)
    print(f"wrote steps_smac_attn.npz: {os.path.getsize(path) / 1024:.1f} KiB, {len(out)} arrays")
