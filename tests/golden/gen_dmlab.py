"""Generate tests/golden/steps_dmlab.npz: the ``dmlab`` policy (IMPALA's DMLab-30 agent) computed by the REAL reference's own
modules (read-only beside this repository), once in float32 and once in float64.

Run (from the repo root):
    CUDA_VISIBLE_DEVICES="" PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout>:. python3 tests/golden/gen_dmlab.py

Harness-side shims (the reference files stay untouched): those of gen_smac_attn.py that concern imports (numpy alias, MagicMock
for absent import-time dependencies, a CPU pass-through for the CUDA prefetcher) and its float64 ones (the network is cast with
``.double()`` after construction; the reference's explicit casts to float32 keep float64 in that run), and one repair:
``_ppo_analyze`` reads the rollout's log-probabilities as ``sample.log_probs`` (dmlab_policy.py:298) where every sample keeps them
at ``sample.analyzed_result.log_probs`` (actor_critic_policy.py reads them there); a ``log_probs`` attribute that falls back to
that leaf is put on ``NamedArray`` while this script runs.  The block cases build
``DMLabActorCritic`` with a smaller vocabulary (the module constant ``DMLAB_VOCABULARY_SIZE`` is set while the case is built) and
read the instruction feature off the input of ``net.rnn``.

Two files, each below the size a committed file may have: ``instr_lstm_blocks.npz`` (the block cases) and ``steps_dmlab.npz`` (the
trainer run).  Float64 quantities are stored as scaled float16 differences to the float32 run (``put64``).  The state dicts after a
step are stored as scaled float16 differences to the snapshot before them, with the error of that encoding beside them (``packq``);
of the float64 run's parameters only their distance to the float32 run is kept (and asserted to stay within the test's tolerance).
The two analyze-only policies take every tensor of equal shape from the trainer's initial state dict and values on a coarse grid
for the others.
"""
import copy
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

DTYPE = [torch.float32]


def _get_log_probs(self):
    return self.__dict__["log_probs"] if "log_probs" in self.__dict__ else self.analyzed_result.log_probs


NamedArray.log_probs = property(_get_log_probs, lambda self, v: self.__dict__.__setitem__("log_probs", v))


class CPUPrefetcher:

    def push(self, sample):
        return sample, recursive_apply(sample, lambda x: torch.from_numpy(x).to(DTYPE[0]))


api.trainer.PyTorchGPUPrefetcher = CPUPrefetcher
import legacy.algorithm.ppo.mappo as mappo

mappo.PyTorchGPUPrefetcher = CPUPrefetcher
from legacy.algorithm.ppo.actor_critic_policies.actor_critic_policy import PPORolloutAnalyzedResult
import legacy.algorithm.ppo.game_policies.dmlab_policy as dmlab  # registers "dmlab"

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from srl_amd.runtime import synthetic


def put64(out, key, v64, v32):
    """out[key + "64d"] (float16) and out[key + "64e"] (k): value64 = float64(value32) + float64(d) * 2 ** -k.  The difference is
    the float32 run's own rounding error; eleven bits of it place the float64 value to ~1e-10 of the tensor's scale."""
    d = np.asarray(v64, np.float64) - np.asarray(v32, np.float64)
    top = float(np.abs(d).max()) if d.size else 0.0
    k = int(9 - np.floor(np.log2(top))) if top > 0 else 0
    out[key + "64d"], out[key + "64e"] = (d * 2.0**k).astype(np.float16), np.array(k)


def pack(out, key, named, named64=None):
    """A name -> array dict as a few arrays: ``key_names``, ``key_shapes`` ([tensors, 4], trailing columns 0) and ``key_flat`` for
    the float32 tensors, ``key_f64:<name>`` for the float64 ones (PopArt's running statistics); with ``named64`` the float64 run's
    values as ``key_flat64d`` / ``key_flat64e`` (``put64`` per tensor, exponents side by side).  tests/dmlab_cases.py has the
    inverse."""
    names = [k for k, v in named.items() if v.dtype != np.float64]
    out[key + "_names"] = np.array(names)
    out[key + "_shapes"] = np.array([tuple(named[k].shape) + (0,) * (4 - named[k].ndim) for k in names])
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


def packq(out, key, named, before, named64):
    """A state dict after a step as scaled float16 differences to the snapshot ``before`` (an Adam step moves a weight by ~lr, so
    eleven bits of the difference place it to ~5e-7): ``key_names`` / ``key_shapes`` as ``pack``, ``key_d`` (float16) and ``key_e``
    per tensor: value = before + d * 2 ** -e.  ``key_q`` is, per tensor, the largest distance of that value to the float32 run's
    true one: the test takes it OFF its tolerance, so the check asks no less than a comparison with the true values would.
    ``key_err64``: per tensor, the largest distance of the float32 run to the float64 run.  float64 tensors (PopArt) as they are."""
    names = [k for k, v in named.items() if v.dtype != np.float64]
    out[key + "_names"] = np.array(names)
    out[key + "_shapes"] = np.array([tuple(named[k].shape) + (0,) * (4 - named[k].ndim) for k in names])
    ds, es, qs, e64, recon = [], [], [], [], {}
    for k in names:
        tmp = {}
        put64(tmp, "x", named[k], np.asarray(before[k], np.float64))
        back = recon[k] = np.asarray(before[k], np.float64) + tmp["x64d"].astype(np.float64) * 2.0**-int(tmp["x64e"])
        ds.append(tmp["x64d"].reshape(-1))
        es.append(int(tmp["x64e"]))
        qs.append(np.abs(back - named[k]).max())
        e64.append(np.abs(named64[k] - named[k]).max())
    out[key + "_d"], out[key + "_e"], out[key + "_q"], out[key + "_err64"] = np.concatenate(ds), np.array(es), np.array(qs), np.array(e64)
    for k, v in named.items():
        if v.dtype == np.float64:
            out[f"{key}_f64:{k}"] = v
    return max(qs), recon   # (the next step's differences are taken to what the reader has: ``recon``)


# ------------------------------------------------------------------------------------------------ block cases
CASES = {  # name: (V, Ed, H, L, rows)
    "a": (50, 20, 64, 6, 37),
    "b": (1000, 20, 64, 16, 130),
    "c": (1000, 20, 64, 1, 5),
    "d": (30, 8, 32, 9, 3),
    "e": (1000, 20, 64, 12, 257),
    "a0": (50, 20, 64, 6, 37),   # case a with a non-zero row 0 of the table
}
BLOCK_PARAMS = ("word_embedding.weight", "instructions_lstm.weight_ih_l0", "instructions_lstm.weight_hh_l0",
                "instructions_lstm.bias_ih_l0", "instructions_lstm.bias_hh_l0")


def block_tokens(name, rng, V, L, n):
    """float32 token ids [n, L] and the row classes the case stands for (asserted)."""
    tok = np.zeros((n, L), dtype=np.int64)
    if name in ("a", "a0"):
        for i in range(n):
            ln = int(rng.integers(1, L + 1))
            tok[i, :ln] = rng.integers(1, V, size=ln)
            if ln < L and rng.random() < 0.4:   # one more token behind a gap: counted, but outside the prefix
                tok[i, min(ln + 1, L - 1)] = rng.integers(1, V)
        tok[0] = 0
        tok[1] = rng.integers(1, V, size=L)
        tok[2] = [5, 0, 7, 0, 0, 0]
        tok[3] = [9, 9, 9, 9, 0, 0]
        tok[4:, 0] = 11
        cnt = (tok != 0).sum(1)
        assert (tok[0] == 0).all() and cnt[1] == L and cnt[2] == 2 and tok[2, 1] == 0 and ((tok == 11).any(1)).sum() >= 32
        assert any(c >= 2 and (tok[i, :c] == 0).any() for i, c in enumerate(cnt))   # a zero inside a prefix
    elif name == "b":
        for i in range(n):
            ln = int(rng.integers(0, L + 1)) if rng.random() < 0.7 else 0
            tok[i, :ln] = rng.integers(1, 40 if i % 2 else V, size=ln)   # a small pool: tokens shared between rows
            if ln >= 3 and rng.random() < 0.3:
                tok[i, int(rng.integers(0, ln - 1))] = 0
        tok[7] = rng.integers(1, V, size=L)
        tok[8, :] = 0
        tok[8, L - 1] = V - 1   # the last table row, alone at the end of the row: length 1, the sequence is [0]
        cnt = (tok != 0).sum(1)
        assert cnt.min() == 0 and cnt.max() == L and len(set(cnt.tolist())) > 8 and (tok == V - 1).any()
    elif name == "c":
        tok[:, 0] = [0, 3, 999, 3, 0]
    elif name == "d":
        pass   # every row empty
    elif name == "e":
        tok[n - 1] = rng.integers(1, V, size=L)
        assert (tok[:-1] == 0).all() and (tok[-1] != 0).all()
    return tok.astype(np.float32)


def gen_block(name, out):
    V, Ed, H, L, n = CASES[name]
    rng = np.random.default_rng(2000 + ord(name[0]))   # a0: the numbers of case a
    hid = 8
    dmlab.DMLAB_VOCABULARY_SIZE = V
    try:
        net = dmlab.DMLabActorCritic({"obs": (1, 20, 20), "INSTR": (L,)}, 3, hid, 0, "lstm", 1, False, "relu", False,
                                     embedding_size=Ed, instrunctions_lstm_units=H)
    finally:
        dmlab.DMLAB_VOCABULARY_SIZE = 1000
    # seeded parameters on a coarse grid (exact in float32, and the file compresses); cases of equal sizes share them
    prng = np.random.default_rng(V * 10000 + Ed * 100 + H)
    with torch.no_grad():
        for k, p in net.named_parameters():
            if k not in BLOCK_PARAMS:
                continue
            g = prng.integers(-24, 25, size=tuple(p.shape)).astype(np.float32) / 64.0
            if k == "word_embedding.weight":
                g = g * 4.0   # ~ the N(0, 1) of nn.Embedding
                if name != "a0":
                    g[0] = 0.0
                else:
                    out["blk_a0_row0"] = g[0].copy()
            elif p.dim() == 2:
                g = g * 2.0**np.round(np.log2(3.0 / np.sqrt(p.shape[1])))
            p.copy_(torch.from_numpy(g.astype(np.float32)))
    tok = block_tokens(name, rng, V, L, n)
    frames = rng.integers(0, 256, size=(1, n, 1, 20, 20)).astype(np.float32)
    cot = rng.integers(-64, 65, size=(n, H)).astype(np.float32) / 64.0
    res = {}
    for tag, dt in (("32", torch.float32), ("64", torch.float64)):
        e = copy.deepcopy(net).to(dt)
        got = []
        e.rnn.register_forward_pre_hook(lambda mod, inp: got.append(inp[0]))   # cat(pixel, instruction) (dmlab_policy.py:160)
        obs = NamedArray(obs=torch.from_numpy(frames).to(dt), INSTR=torch.from_numpy(tok[None]).to(dt))
        e(obs, torch.zeros(1, n, hid, dtype=dt), torch.zeros(1, n, 1, dtype=dt))
        feat = got[0][0, :, hid:]
        assert feat.shape == (n, H)
        (feat * torch.from_numpy(cot).to(dt)).sum().backward()
        grads = {k: p.grad.numpy() for k, p in e.named_parameters() if k in BLOCK_PARAMS}
        assert not grads["word_embedding.weight"][0].any()   # padding_idx: row 0 collects nothing
        res[tag] = (feat.detach().numpy(), grads)
    pre = f"blk_{name}_"
    out[pre + "dims"] = np.array([V, Ed, H, L, n])
    out[pre + "tok"], out[pre + "cot"] = tok, cot
    if f"par_{V}_{Ed}_{H}_names" not in out:   # (case a0: these with ``blk_a0_row0`` as row 0 of the table)
        assert name != "a0"
        pack(out, f"par_{V}_{Ed}_{H}", {k: p.detach().numpy() for k, p in net.named_parameters() if k in BLOCK_PARAMS})
    out[pre + "out32"] = res["32"][0]
    put64(out, pre + "out", res["64"][0], res["32"][0])
    pack(out, pre + "grad", res["32"][1], res["64"][1])
    err = max(np.abs(res["64"][1][k] - res["32"][1][k]).max() / max(np.abs(res["64"][1][k]).max(), 1e-30) for k in res["32"][1])
    cnt = (tok != 0).sum(1)
    print(f"block {name}: rows {n} empty rows {(cnt == 0).sum()} longest {cnt.max()}, float32 gradient error (rel. to max) {err:.2e}, "
          f"output error {np.abs(res['64'][0] - res['32'][0]).max():.2e}")


# ------------------------------------------------------------------------------------------------ trainer run
HID, CL, ACT, L, SEED = 64, 5, 9, 6, 31
OBS = {"obs": (3, 36, 44), "INSTR": (L,)}
POLICY = dict(obs_shapes=OBS, action_dim=ACT, hidden_dim=HID, chunk_len=CL, seed=SEED)
TRAINER = dict(popart=True, ppo_epochs=2, optimizer_config=dict(lr=5e-4, eps=1e-5), max_grad_norm=10.0,
               value_loss="huber", value_loss_config=dict(delta=10.0), clip_value=True, dual_clip=False)
SAMPLE = dict(T=10, B=3, obs_spec={"obs": ((3, 36, 44), "u8")}, action_dims=ACT, p_done=0.08)
PARAM_TOL = 2e-5


def instructions(rng, lead):
    """float32 token ids [*lead, L]: four in ten rows empty, the others 1..L tokens of a small pool, some with a gap."""
    n = int(np.prod(lead))
    tok = np.zeros((n, L), dtype=np.int64)
    for i in range(n):
        if rng.random() < 0.4:
            continue
        ln = int(rng.integers(1, L + 1))
        tok[i, :ln] = rng.integers(1, 30 if rng.random() < 0.7 else 1000, size=ln)
        if ln >= 3 and rng.random() < 0.3:
            tok[i, 1] = 0
    return tok.reshape(*lead, L).astype(np.float32)


def make_arrays(seed, state=(1, HID)):
    arrays = synthetic.make_sample_arrays(seed=seed, policy_state={"hx": state} if state else None, **SAMPLE)
    arrays["obs.INSTR"] = instructions(np.random.default_rng(seed + 77), arrays["on_reset"].shape[:2])
    return arrays


def ref_sample(arrays):
    hx = arrays.get("policy_state.hx")
    return api.trainer.SampleBatch(obs=NamedArray(obs=arrays["obs.obs"], INSTR=arrays["obs.INSTR"]),
                                   policy_state=NamedArray(hx=hx) if hx is not None else None,
                                   on_reset=arrays["on_reset"], done=arrays["done"], truncated=arrays["truncated"],
                                   action=DiscreteAction(arrays["action.x"]), reward=arrays["reward"],
                                   analyzed_result=PPORolloutAnalyzedResult(log_probs=arrays["analyzed_result.log_probs"],
                                                                            value=arrays["analyzed_result.value"]),
                                   policy_version_steps=arrays["policy_version_steps"], info_mask=arrays["info_mask"])


def sd_np(net):
    return {k: v.detach().cpu().numpy().copy() for k, v in net.state_dict().items()}


def analyze(policy, arrays, dt):
    ts = recursive_apply(ref_sample({k: v.copy() for k, v in arrays.items()}), lambda x: torch.from_numpy(x).to(dt))
    Tb = arrays["on_reset"].shape[0]
    with torch.no_grad():
        ar = policy.analyze(ts[:Tb - 1], target="ppo", burn_in_steps=0)
    return ar.new_action_log_probs.numpy(), ar.state_values.numpy(), ar.entropy.numpy()


def run_trainer(dt):
    DTYPE[0] = dt
    r = {}
    trainer = api.trainer.make(api.config.Trainer("mappo", args=TRAINER), api.config.Policy("dmlab", args=POLICY))
    if dt == torch.float64:
        trainer.policy.net.double()  # the float32 initial values, exactly; the optimiser keeps the same Parameter objects
    net = trainer.policy.net
    r["init"] = sd_np(net)
    for step in range(2):
        arrays = make_arrays(500 + step)
        r[f"instr{step}"] = arrays["obs.INSTR"]
        if step == 0:
            r["analyze"] = analyze(trainer.policy, arrays, dt)
        sample = ref_sample({k: v.copy() for k, v in arrays.items()})
        res = trainer.step(sample)
        stats = {k: float(v) for k, v in res.stats.items()}
        r["stat_names"] = sorted(stats)
        r[f"stats{step}"] = np.array([stats[k] for k in r["stat_names"]], dtype=np.float64)
        if step == 0:
            r["adv"], r["ret"] = np.asarray(sample.analyzed_result.adv), np.asarray(sample.analyzed_result.ret)
        r[f"param{step}"] = sd_np(net)
    r["version"] = trainer.policy.version
    # deterministic rollout of 5 requests with the trained weights
    policy = trainer.policy
    rng = np.random.default_rng(12)
    N = 5
    frames = rng.integers(0, 256, size=(N, 3, 36, 44), dtype=np.uint8)
    instr = instructions(rng, (N,))
    instr[0], instr[1] = 0, [4, 0, 9, 0, 0, 0]
    hx = (0.5 * rng.standard_normal((N, 1, HID))).astype(np.float32)
    on_reset = (rng.random((N, 1)) < 0.4).astype(np.uint8)
    aux = {k: np.zeros((N, 1), dtype=np.int32) for k in ("client_id", "request_id", "received_time", "buffer_index", "step_count",
                                                          "ready")}
    rr = api.policy.RolloutRequest(obs=NamedArray(obs=frames, INSTR=instr), policy_state=NamedArray(hx=hx),
                                   is_evaluation=np.ones((N, 1), dtype=np.uint8), on_reset=on_reset, **aux)
    if dt == torch.float64:  # the reference's rollout casts its requests to float32 (dmlab_policy.py:322-323): keep the float64 net
        orig = torch.Tensor.to
        with mock.patch.object(torch.Tensor, "to", lambda self, *a, **k: orig(self, *a, **{**k, "dtype": dt}) if k.get("dtype") == torch.float32 else orig(self, *a, **k)):
            res = policy.rollout(rr)
    else:
        res = policy.rollout(rr)
    r["roll_in"] = dict(obs=frames, INSTR=instr, hx=hx, on_reset=on_reset)
    r["roll"] = dict(action=res.action.x, log_probs=res.analyzed_result.log_probs, value=res.analyzed_result.value,
                     new_hx=res.policy_state.hx)
    return r


def gen_variant(out, tag, init, extra_args, state):
    """One analyze-only policy: every tensor whose name and shape the trainer's initial state dict has is taken from there."""
    DTYPE[0] = torch.float32
    policy = api.policy.make(api.config.Policy("dmlab", args=dict(POLICY, **extra_args)))
    sd = policy.net.state_dict()
    shared = {k: torch.from_numpy(init[k]) for k, v in sd.items() if k in init and tuple(init[k].shape) == tuple(v.shape)}
    policy.net.load_state_dict(shared, strict=False)
    rng = np.random.default_rng(len(tag))
    with torch.no_grad():   # its own tensors: the initial values rounded to multiples of 1/256 (the file compresses)
        for k, p in policy.net.named_parameters():
            if k not in shared:
                p.copy_(torch.round(p * 256.0) / 256.0 + torch.from_numpy(rng.integers(-2, 3, size=tuple(p.shape)) / 256.0).float())
    own = {k: v for k, v in sd_np(policy.net).items() if k not in shared}
    arrays = make_arrays(500, state)
    lp, val, ent = analyze(policy, arrays, torch.float32)
    pack(out, f"{tag}_init", own)
    if state:
        out[f"{tag}_hx"] = arrays["policy_state.hx"]
    out[f"{tag}_new_lp"], out[f"{tag}_value"], out[f"{tag}_entropy"] = lp, val, ent
    print(f"{tag}: {len(shared)} shared tensors, {len(own)} of its own ({sum(v.size for v in own.values())} values)")


def gen_trainer(out):
    r32 = run_trainer(torch.float32)
    # float64 run: the reference casts to float32 at a few places (gae.py:97, utils.py:67,144,151); `.float()` keeps float64 here
    with mock.patch.object(torch.Tensor, "float", lambda self: self.double()):
        r64 = run_trainer(torch.float64)
    pack(out, "init", r32["init"])
    for k, v in r32["init"].items():
        assert np.array_equal(np.asarray(r64["init"][k], np.float64), np.asarray(v, np.float64)), k
    print(f"state dict: {len(r32['init'])} tensors, {sum(v.size for v in r32['init'].values())} values: {list(r32['init'])}")
    out["stat_names"], out["version"] = np.array(r32["stat_names"]), np.array(r32["version"])
    for i, name in enumerate(("new_lp", "value", "entropy")):
        out[f"analyze_{name}"] = r32["analyze"][i]
        put64(out, f"analyze_{name}", r64["analyze"][i], r32["analyze"][i])
    out["step0_adv"], out["step0_ret"] = r32["adv"], r32["ret"]
    put64(out, "step0_adv", r64["adv"], r32["adv"])
    put64(out, "step0_ret", r64["ret"], r32["ret"])
    before = r32["init"]
    for step in range(2):
        out[f"sample{step}.obs.INSTR"] = r32[f"instr{step}"]
        out[f"step{step}_stats"], out[f"step{step}_stats64"] = r32[f"stats{step}"], r64[f"stats{step}"]
        q, before = packq(out, f"step{step}", r32[f"param{step}"], before, r64[f"param{step}"])
        print(f"step {step}: the encoding places the parameters to {q:.2e}")
        worst = max((np.abs(r64[f"param{step}"][k] - v).max(), k) for k, v in r32[f"param{step}"].items() if v.dtype != np.float64)
        print(f"step {step}: the float32 run's largest parameter difference to the float64 run {worst[0]:.3e} at {worst[1]}")
        assert worst[0] <= PARAM_TOL, "pick another seed: the reference's own float32 run leaves the parameter tolerance"
    for k, v in r32["roll_in"].items():
        out[f"roll_in.{k}"] = v
    for k, v in r32["roll"].items():
        out[f"roll_{k}"] = np.asarray(v)
        if k != "action":
            put64(out, f"roll_{k}", r64["roll"][k], v)
    assert np.array_equal(r32["roll"]["action"], r64["roll"]["action"])
    gen_variant(out, "gru", r32["init"], dict(hidden_dim=32, rnn_type="gru"), (1, 16))
    gen_variant(out, "nornn", r32["init"], dict(num_rnn_layers=0), None)


def save(name, out):
    out["torch_version"] = np.array(torch.__version__)
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **out)
    print(f"wrote {name}: {os.path.getsize(path) / 1024:.1f} KiB, {len(out)} arrays")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    out = {}
    for name in CASES:
        gen_block(name, out)
    save("instr_lstm_blocks.npz", out)
    out = {}
    gen_trainer(out)
    save("steps_dmlab.npz", out)
