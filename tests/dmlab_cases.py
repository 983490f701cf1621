"""Shared by the ``dmlab`` tests: the shapes of tests/golden/gen_dmlab.py, readers of its packed arrays, and a plain torch restatement
of the network (``DMLabOracle``) that tests/test_gpu_dmlab.py runs in float32 and float64 through ``oracle.trainer.OracleMappo``."""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from srl_amd.namedarray import NamedArray
from srl_amd.runtime import synthetic

HID, CL, ACT, L, SEED = 64, 5, 9, 6, 31
OBS = {"obs": (3, 36, 44), "INSTR": (L,)}
POLICY = dict(obs_shapes=OBS, action_dim=ACT, hidden_dim=HID, chunk_len=CL, seed=SEED)
GRU_POLICY = dict(POLICY, hidden_dim=32, rnn_type="gru")
NORNN_POLICY = dict(POLICY, num_rnn_layers=0)
TRAINER = dict(popart=True, ppo_epochs=2, optimizer_config=dict(lr=5e-4, eps=1e-5), max_grad_norm=10.0,
               value_loss="huber", value_loss_config=dict(delta=10.0), clip_value=True, dual_clip=False)
SAMPLE = dict(T=10, B=3, obs_spec={"obs": ((3, 36, 44), "u8")}, action_dims=ACT, p_done=0.08)
PARAM_TOL = 2e-5   # parameters after a step (tests/test_gpu_smac_attn.py)
BLOCKS = ("a", "b", "c", "d", "e")
BLOCK_PARAMS = OrderedDict(emb="word_embedding.weight", w_ih="instructions_lstm.weight_ih_l0", w_hh="instructions_lstm.weight_hh_l0",
                           b_ih="instructions_lstm.bias_ih_l0", b_hh="instructions_lstm.bias_hh_l0")


def unpack(g, key, f64=False):
    """name -> array of a dict stored by gen_dmlab.pack; ``f64``: the float64 run's values instead."""
    out, off = OrderedDict(), 0
    flat = g[key + "_flat"]
    for i, (name, shp) in enumerate(zip(g[key + "_names"], g[key + "_shapes"])):
        shp = tuple(int(x) for x in shp if x)
        n = int(np.prod(shp))
        v = flat[off:off + n].reshape(shp)
        if f64:
            v = v.astype(np.float64) + g[key + "_flat64d"][off:off + n].astype(np.float64).reshape(shp) * 2.0**-int(g[key + "_flat64e"][i])
        out[str(name)] = v
        off += n
    return out


def state_dict(g, key):
    """The float32 tensors of ``unpack`` and the float64 PopArt statistics stored beside them."""
    sd = OrderedDict(unpack(g, key))
    for k in g.files:
        if k.startswith(key + "_f64:"):
            sd[k[len(key) + 5:]] = g[k]
    return sd


def state_after(g, step):
    """(state dict after trainer step ``step``, per-tensor distance of these values to the float32 run's true ones): stored by
    gen_dmlab.packq as scaled float16 differences to the snapshot before.  float32 tensors come back as float64 arrays."""
    before = {k: v.astype(np.float64) for k, v in unpack(g, "init").items()} if step == 0 else state_after(g, step - 1)[0]
    key = f"step{step}"
    sd, q, off = OrderedDict(), {}, 0
    for i, (name, shp) in enumerate(zip(g[key + "_names"], g[key + "_shapes"])):
        name, shp = str(name), tuple(int(x) for x in shp if x)
        n = int(np.prod(shp))
        sd[name] = before[name] + g[key + "_d"][off:off + n].astype(np.float64).reshape(shp) * 2.0**-int(g[key + "_e"][i])
        q[name] = float(g[key + "_q"][i])
        off += n
    return sd, q


def popart_after(g, step):
    key = f"step{step}_f64:"
    return {k[len(key):]: g[k] for k in g.files if k.startswith(key)}


def variant_state(g, tag, names):
    """State dict of an analyze-only policy with the tensors ``names``: its own where the file has them, else the trainer's
    initial ones (gen_dmlab.gen_variant took every tensor of equal name and shape from there)."""
    init, own = state_dict(g, "init"), state_dict(g, f"{tag}_init")
    return OrderedDict((k, own[k] if k in own else init[k]) for k in names)


def get64(g, key, base=None):
    """The float64 run's value of a quantity stored by gen_dmlab.put64 (``base``: the name of its float32 array)."""
    return g[base or key].astype(np.float64) + g[key + "64d"].astype(np.float64) * 2.0**-int(g[key + "64e"])


def block_params(g, name):
    """The five parameters of a block case (shared between the cases of equal sizes; case a0: a non-zero row 0)."""
    V, Ed, H, _, _ = (int(x) for x in g[f"blk_{name}_dims"])
    p = {k: v.copy() for k, v in unpack(g, f"par_{V}_{Ed}_{H}").items()}
    if name == "a0":
        p["word_embedding.weight"][0] = g["blk_a0_row0"]
    return p


def make_arrays(g, step, state=(1, HID)):
    """The flat sample of gen_dmlab.make_arrays: synthetic leaves by seed, the instructions from the file."""
    arrays = synthetic.make_sample_arrays(seed=500 + step, policy_state={"hx": state} if state else None, **SAMPLE)
    arrays["obs.INSTR"] = g[f"sample{step}.obs.INSTR"]
    return arrays


def make_sample(g, step, state=(1, HID)):
    arrays = make_arrays(g, step, state)
    return synthetic.to_sample_batch(arrays), arrays


class DMLabOracle:
    """The ``dmlab`` network and its PPO analysis in plain torch (autograd), in ``dtype``: a restatement from the issue's
    description (pixels / 255 -> conv 8/4 -> conv 4/2 -> Linear; the first max(1, #non-zero) tokens through Embedding + LSTM; their
    concatenation through the auto-reset LSTM from the chunk's stored state; linear heads), with the interface
    ``oracle.trainer.OracleMappo`` and ``rnn_ref.check_vs_float64`` use."""
    shared, num_rnn_layers, popart = True, 1, False

    def __init__(self, sd, chunk_len, dtype):
        self.dtype, self.chunk_len = dtype, chunk_len
        self.params = OrderedDict((k, torch.as_tensor(np.asarray(v)).to(dtype).clone().requires_grad_(True)) for k, v in sd.items()
                                  if "_RunningMeanStd__" not in k)

    def parameters(self):
        return list(self.params.values())

    @staticmethod
    def _lstm_step(x, h, c, w_ih, w_hh, b_ih, b_hh):
        i, f, g, o = (x @ w_ih.T + b_ih + h @ w_hh.T + b_hh).chunk(4, -1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        return torch.sigmoid(o) * torch.tanh(c), c

    def _instr(self, tok):
        p = self.params
        tok = tok.long()
        n, U = tok.shape[0], p["instructions_lstm.weight_hh_l0"].shape[1]
        lens = (tok != 0).sum(-1).clamp(min=1)
        h = c = torch.zeros(n, U, dtype=self.dtype)
        for t in range(int(lens.max())):
            x = F.embedding(tok[:, t], p["word_embedding.weight"], padding_idx=0)   # (row 0 is read, and collects no gradient)
            h2, c2 = self._lstm_step(x, h, c, *(p[f"instructions_lstm.{k}_l0"] for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")))
            on = (t < lens).to(self.dtype).unsqueeze(-1)
            h, c = on * h2 + (1 - on) * h, on * c2 + (1 - on) * c
        return h

    def forward(self, obs, state, on_reset):
        p = self.params
        T, B = on_reset.shape[:2]
        x = obs["obs"].reshape(T * B, *obs["obs"].shape[2:]) / 255.0
        x = torch.relu(F.conv2d(x, p["pixel_encoder.0.weight"], p["pixel_encoder.0.bias"], stride=4))
        x = torch.relu(F.conv2d(x, p["pixel_encoder.2.weight"], p["pixel_encoder.2.bias"], stride=2))
        x = F.linear(x.flatten(1), p["pixel_encoder.5.weight"], p["pixel_encoder.5.bias"])
        feat = torch.cat([x, self._instr(obs["INSTR"].reshape(T * B, -1))], -1).reshape(T, B, -1)
        R = p["rnn._AutoResetRNN__net.weight_hh_l0"].shape[1]
        h, c = state[0][0, :, :R], state[0][0, :, R:]
        ys = []
        for t in range(T):
            keep = 1 - on_reset[t]
            h, c = self._lstm_step(feat[t], h * keep, c * keep, *(p[f"rnn._AutoResetRNN__net.{k}_l0"]
                                                                    for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")))
            ys.append(h)
        y = torch.stack(ys)
        head = "critic_head._PopArtValueHead__" if "critic_head._PopArtValueHead__weight" in p else "critic_head."
        return (F.linear(y, p["actor_head.weight"], p["actor_head.bias"]), F.linear(y, p[head + "weight"], p[head + "bias"]), None)

    def analyze(self, obs, action, on_reset, policy_state=None, burn_in_steps=0):
        assert burn_in_steps == 0
        T = on_reset.shape[0]
        n = T // self.chunk_len
        chunk = lambda x: torch.cat(torch.split(x, T // n, dim=0), dim=1)
        unchunk = lambda x: torch.cat(torch.split(x, x.shape[1] // n, dim=1), dim=0)
        state = tuple(chunk(s)[0].transpose(0, 1) for s in policy_state)
        logits, value, _ = self.forward({k: chunk(v) for k, v in obs.items()}, state, chunk(on_reset))
        logits, value = unchunk(logits), unchunk(value)
        dist = torch.distributions.Categorical(logits=logits)
        return dist.log_prob(action[..., 0]).unsqueeze(-1), value, dist.entropy().unsqueeze(-1), logits


def rollout_request(g):
    from srl_amd.api import policy as policy_api
    pre = "roll_in."
    N = g[pre + "on_reset"].shape[0]
    return policy_api.RolloutRequest(obs=NamedArray(obs=g[pre + "obs"], INSTR=g[pre + "INSTR"]), policy_state=NamedArray(hx=g[pre + "hx"]),
                                     is_evaluation=np.ones((N, 1), np.uint8), on_reset=g[pre + "on_reset"]), N
