"""``atari-dqn``: the dueling double-DQN agent on the HIP kernels.

Mirror of ``AtariDQNPolicy`` (reference ``legacy/algorithm/q_learning/game_policies/atari_dqn_policy.py:117-302``): the same
constructor keywords and defaults, the same ``state_dict`` names (``net.conv1.weight`` ... ``net.fc_v.2.bias``, then the same under
``target_net.``), ``analyze(target="dqn", burn_in_steps=...)`` and ``rollout``, ``soft_target_update`` / ``hard_target_update``.

The online and the target network are two executors over two parameter sets of one ``NetSpec``
(``netspec.build_atari_dqn_netspec``); the convolution trunk runs once per pass per network, both towers' first Linear being one
product.  ``analyze`` does not gather: it returns both networks' head outputs for every row, and the trainer's TD kernel
(``csrc/dqn.hip``) forms Q, the greedy action and the gathers itself.  ``rollout`` samples with ``srl_epsilon_greedy_sample``
(``csrc/dqn.hip`` too; its Philox draw is ``csrc/action_dist.h``'s, the one the action heads' samplers use).

With ``num_rnn_layers > 0`` the agent is the recurrent one (R2D2): an auto-reset GRU / LSTM between the trunk and the towers
(``algorithm/rnnpath.py``), chunks of ``chunk_len`` steps starting from the stored ``policy_state.hx``, and -- with
``burn_in_steps`` -- a burn-in pass through the online network that gives both networks their initial state (``burn_in_plan``).

DIFFERENCES: exploration draws come from a counter-based Philox stream keyed by ``(seed, call counter)`` instead of torch's
generator.  The reference's recurrent towers read 512 columns whatever ``hidden_dim`` is (:70), so it runs only at
``hidden_dim=512``, and so does this policy by default: another width with ``num_rnn_layers > 0`` raises.  The extra keyword
``rnn_towers_read_hidden_dim=True`` is this project's extension: towers that read ``hidden_dim`` columns (the reference at 512),
at any multiple of 4 -- it exists so that the small-width chunk kernels can be tested under this agent.
``dueling=False``, ``rnn_type='gtrxl'``, ``rnn_include_last_action`` / ``rnn_include_last_reward`` and data parallelism raise
``NotImplementedError``.
"""
import dataclasses
from collections import OrderedDict
from typing import NamedTuple, Optional

import numpy as np
import torch

from srl_amd import hip
from srl_amd.algorithm import netspec as ns
from srl_amd.algorithm.actor_critic import to_device_leaf
from srl_amd.algorithm.hipnet import HipNet, RnnCtx
from srl_amd.api import policy as policy_api
from srl_amd.api.env_utils import DiscreteAction
from srl_amd.namedarray import NamedArray


class DQNPolicyState(policy_api.PolicyState, NamedArray):

    def __init__(self, hx: np.ndarray, epsilon: np.ndarray):
        super().__init__(hx=hx, epsilon=epsilon)


class DQNRolloutAnalyzedResult(policy_api.AnalyzedResult, NamedArray):

    def __init__(self, value: np.ndarray, target_value: np.ndarray, ret: Optional[np.ndarray] = None):
        super().__init__(value=value, target_value=target_value, ret=ret)


@dataclasses.dataclass
class DQNHeadOutputs:
    """``analyze(target="dqn")``: both networks' head outputs for the ``T x B`` rows behind the burn-in steps, time-major
    (row = t * B + b) -- what ``hip.dqn_td_fwd_bwd`` reads.  The online outputs are on the tape: ``backward_dqn`` follows."""
    adv: torch.Tensor  # [T*B, A] online advantages
    value: torch.Tensor  # [T*B, 1] online state values
    target_adv: torch.Tensor  # [T*B, A]
    target_value: torch.Tensor  # [T*B, 1]
    action: torch.Tensor  # int32 [T*B]
    T: int
    B: int


BurnInPlan = NamedTuple("BurnInPlan", [("num_chunks", int), ("chunk", int), ("windows", list), ("state_rows", list)])


def burn_in_plan(sample_rows: int, burn_in_steps: int, chunk_len: int) -> BurnInPlan:
    """The index arithmetic of ``_dqn_analyze`` (:168-193) for a sample of ``sample_rows`` steps: the ``T = sample_rows -
    burn_in_steps`` analysed steps are ``num_chunks = T // chunk_len`` chunks of ``chunk = T / num_chunks`` steps (chunk ``k`` is rows
    ``[burn + k chunk, burn + (k + 1) chunk)`` of the sample; column ``k B + b`` of a recurrent pass).  ``state_rows[k]``: the row of
    the sample whose stored ``policy_state.hx`` starts chunk ``k``'s first pass.  Without burn-in that is the chunk's first row and
    ``windows`` is empty.  With burn-in, ``windows[k] = (k chunk_len, k chunk_len + burn)`` are the rows of the FULL sample the
    online network replays first, from the state stored at ``k chunk_len``: the reference's literal indices (:183).  They end right
    in front of chunk ``k`` only when ``chunk == chunk_len``; otherwise (44 analysed steps with ``chunk_len=40``: one chunk of 44;
    10 with ``chunk_len=4``: two of 5) the later windows start ``k (chunk - chunk_len)`` rows early, as in the reference."""
    burn, cl = int(burn_in_steps), int(chunk_len)
    T = int(sample_rows) - burn
    K = max(T, 0) // cl  # (:169-173: 44 steps with chunk_len=40 are one chunk of 44)
    if K == 0 or T % K:
        raise ValueError(f"atari-dqn: {sample_rows} steps less {burn} burn-in steps do not split into {K} equal chunks "
                         f"(chunk_len={cl})")
    C = T // K
    if not burn:
        return BurnInPlan(K, C, [], [k * C for k in range(K)])
    return BurnInPlan(K, C, [(k * cl, k * cl + burn) for k in range(K)], [k * cl for k in range(K)])


class AtariDQNPolicy(policy_api.Policy):

    def __init__(self,
                 act_dim: int,
                 dueling: bool,
                 chunk_len: int = 40,
                 use_double_q: bool = True,
                 seed: int = 42,
                 num_rnn_layers: int = 0,
                 hidden_dim: int = 512,
                 rnn_type: str = 'gru',
                 rnn_include_last_action: bool = False,
                 rnn_include_last_reward: bool = False,
                 use_env_epsilon: bool = True,
                 epsilon_scheduler=None,
                 rnn_towers_read_hidden_dim: bool = False):
        super().__init__()
        if not dueling:
            raise NotImplementedError("atari-dqn: dueling=False is not implemented on the HIP path (the kernels form "
                                      "Q = v + adv - mean adv themselves)")
        if num_rnn_layers > 0 and rnn_type == "gtrxl":
            raise NotImplementedError("atari-dqn: rnn_type='gtrxl' is not implemented on the HIP path (only the GRU and LSTM "
                                      "cells of AutoResetRNN are)")
        if num_rnn_layers > 0 and rnn_type not in ("gru", "lstm"):
            raise NotImplementedError(f"RNN type {rnn_type} has not been implemented.")  # autoreset_rnn.py:27
        if num_rnn_layers > 0 and (rnn_include_last_action or rnn_include_last_reward):
            raise NotImplementedError("atari-dqn: rnn_include_last_action / rnn_include_last_reward (extra input columns of the "
                                      "recurrent layer) are not implemented on the HIP path")
        if num_rnn_layers > 0 and int(hidden_dim) != 512 and not rnn_towers_read_hidden_dim:
            raise NotImplementedError(f"atari-dqn: the reference's recurrent towers read 512 columns whatever hidden_dim is (:70), so "
                                      f"its recurrent agent exists at hidden_dim=512 only (got {hidden_dim}); "
                                      "rnn_towers_read_hidden_dim=True builds this project's extension, towers that read hidden_dim")
        if num_rnn_layers > 0 and torch.distributed.is_available() and torch.distributed.is_initialized():
            raise NotImplementedError("atari-dqn: data-parallel training of the recurrent agent is not implemented (a process "
                                      "group is initialised)")
        if not use_env_epsilon and epsilon_scheduler is None:
            raise ValueError("atari-dqn: use_env_epsilon=False needs an epsilon_scheduler (an object with `get(step)`)")
        np.random.seed(seed)  # atari_dqn_policy.py:134
        self.spec, init = ns.build_atari_dqn_netspec(int(act_dim), hidden_dim, seed=seed, num_rnn_layers=int(num_rnn_layers),
                                                     rnn_type=rnn_type)
        self._net = HipNet(self.spec, self.device)
        self._net.load_reference_state(init)
        # the target network: its own parameter state; it takes no gradient and keeps no tape
        self._target = HipNet(self.spec, self.device)
        self._target.grad = self._target.grad[:0]
        self._target.load_reference_state(init)
        self.use_double_q = bool(use_double_q)
        self._act_dim = int(act_dim)
        self._chunk_len = int(chunk_len)
        self._use_env_epsilon = bool(use_env_epsilon)
        self._exploration = epsilon_scheduler
        hx = np.zeros((self.spec.num_rnn_layers, self.spec.rnn_state_width), dtype=np.float32) if num_rnn_layers > 0 else None  # :140
        self._default_policy_state = DQNPolicyState(hx=hx, epsilon=np.ones(1, dtype=np.float32))
        self._version = -1
        self._seed = int(seed)
        self._rollout_calls = 0
        self._analysis = None

    # ------------------------------------------------------------------ bookkeeping (api/policy.py:205-288)
    @property
    def default_policy_state(self):
        return self._default_policy_state

    @property
    def version(self) -> int:
        return self._version

    @property
    def net(self) -> HipNet:
        return self._net

    @property
    def target_net(self) -> HipNet:
        return self._target

    def inc_version(self):
        self._version += 1

    def parameters(self):
        return [self._net.flat]

    def train_mode(self):
        pass

    def eval_mode(self):
        pass

    def distributed(self):
        if torch.distributed.is_initialized():
            raise NotImplementedError("atari-dqn: data-parallel training is not implemented")

    def get_checkpoint(self):
        sd = OrderedDict((f"net.{k}", v) for k, v in self._net.reference_state().items())
        sd.update((f"target_net.{k}", v) for k, v in self._target.reference_state().items())
        return {"steps": self._version, "state_dict": sd}

    def load_checkpoint(self, checkpoint):
        sd = checkpoint["state_dict"]
        parts = {"net.": {}, "target_net.": {}}
        for k, v in sd.items():
            pre = next((p for p in parts if k.startswith(p)), None)
            if pre is None:
                raise KeyError(f"state_dict mismatch: unexpected {k}")
            parts[pre][k[len(pre):]] = v
        self._net.load_reference_state(parts["net."])
        self._target.load_reference_state(parts["target_net."])
        self._version = checkpoint.get("steps", 0)

    # ------------------------------------------------------------------ target network (atari_dqn_policy.py:295-299)
    def soft_target_update(self, tau):
        hip.require_gpu()
        hip.polyak_update(self._target.flat, self._net.flat, tau)
        self._target.params_changed()

    def hard_target_update(self):
        self.soft_target_update(1.0)

    # ------------------------------------------------------------------ training-side analysis
    def analyze(self, sample, target="dqn", **kwargs):
        if target == "dqn":
            return self._dqn_analyze(sample, **kwargs)
        raise NotImplementedError(f"Unkown analyze target {target}.")

    def _dqn_analyze(self, sample, burn_in_steps=0) -> DQNHeadOutputs:
        """Rows [burn_in_steps, Tb) of ``sample`` (leaves ``[Tb, B, ...]``) through both networks (:168-236).  Without a recurrent
        layer the reference's chunking only permutes independent rows, so they are evaluated in place; its shape requirement
        (``modules/utils.py:176``) is kept.  With one, the passes run in the reference's order -- burn-in through the online
        network (no tape; ``burn_in_plan``), target (no tape), online (tape) -- and the burn-in's final state starts both others."""
        hip.require_gpu()
        burn = int(burn_in_steps)
        Tb, B = sample.on_reset.shape[0], sample.on_reset.shape[1]
        T = Tb - burn
        plan = burn_in_plan(Tb, burn, self._chunk_len)
        n = T * B
        full = to_device_leaf(sample.obs.obs, self.device, "obs")
        frames = full[burn:]
        obs = {"obs": frames.reshape(n, *frames.shape[2:])}
        action = to_device_leaf(sample.action.x, self.device, "index")[burn:].reshape(n)
        ctx = None
        if self.spec.num_rnn_layers:
            ctx = self._recurrent_ctx(sample, full, plan, burn, Tb, B)
        tadv, tv = self._target.forward(obs, n, keep_tape=False, rnn=ctx)
        adv, v = self._net.forward(obs, n, keep_tape=True, rnn=ctx)
        self._analysis = n
        return DQNHeadOutputs(adv, v, tadv, tv, action, T, B)

    def _recurrent_ctx(self, sample, full, plan: BurnInPlan, burn, Tb, B) -> RnnCtx:
        """The time structure of the analysed rows and each chunk's initial state: the stored one, or what the burn-in pass leaves."""
        L, SW, K, C = self.spec.num_rnn_layers, self.spec.rnn_state_width, plan.num_chunks, plan.chunk
        ps = sample.policy_state
        if ps is None or ps.hx is None:
            raise ValueError("atari-dqn: the recurrent agent's sample carries no policy_state.hx")
        hx = to_device_leaf(ps.hx, self.device, "real").reshape(Tb, B, L, SW)
        on_reset = to_device_leaf(sample.on_reset, self.device, "flag").reshape(Tb, B)
        stored = torch.stack([hx[r] for r in plan.state_rows]).reshape(K * B, L, SW).permute(1, 0, 2).contiguous()  # column k B + b
        if plan.windows:
            w_frames = torch.cat([full[a:b] for a, b in plan.windows], dim=0)   # [K burn, B, ...]: chunk k of the pass = window k
            w_reset = torch.stack([on_reset[a:b] for a, b in plan.windows]).permute(1, 0, 2).reshape(burn, K * B).contiguous()
            m = K * burn * B
            self._net.forward({"obs": w_frames.reshape(m, *w_frames.shape[2:])}, m, keep_tape=False,
                              rnn=RnnCtx(K * burn, B, burn, {"a:": stored}, w_reset))
            stored = self._net.last_state["a:"].clone()
        reset = on_reset[burn:].reshape(K, C, B).permute(1, 0, 2).reshape(C, K * B).contiguous()
        return RnnCtx(Tb - burn, B, C, {"a:": stored}, reset)

    def backward_dqn(self, d_adv: torch.Tensor, d_v: torch.Tensor):
        """Back-propagate d loss / d (advantages, state values) of the last ``analyze`` into ``net.grad``."""
        n = self._analysis
        self._net.backward(d_adv.reshape(n, -1), d_v.reshape(n, 1))
        self._analysis = None

    # ------------------------------------------------------------------ inference (:238-289)
    def rollout(self, requests: policy_api.RolloutRequest, **kwargs) -> policy_api.RolloutResult:
        hip.require_gpu()
        frames = requests.obs.obs
        if frames.dtype not in (np.uint8, torch.uint8):
            raise AssertionError(frames.dtype)  # :240
        n = int(frames.shape[0])
        if self._use_env_epsilon:  # the environment provides epsilon as an observation
            eps_host = np.asarray(requests.obs.epsilon, dtype=np.float32).reshape(n, 1)
        else:
            eps_host = np.full((n, 1), self._exploration.get(max(0, self.version)), dtype=np.float32)
        is_eval = np.asarray(requests.is_evaluation).reshape(-1)
        is_eval = to_device_leaf(np.broadcast_to(is_eval, (n,)) if is_eval.size == 1 else is_eval, self.device, "flag")
        obs = {"obs": to_device_leaf(frames, self.device, "obs")}
        eps = to_device_leaf(eps_host, self.device, "real").reshape(n)
        ctx = None
        if self.spec.num_rnn_layers:   # [n, layers, SW] in and out; on_reset masks the INCOMING state (:250-252), for both networks
            L, SW = self.spec.num_rnn_layers, self.spec.rnn_state_width
            ps = requests.policy_state
            if ps is None or ps.hx is None:
                raise ValueError("atari-dqn: the recurrent agent's request carries no policy_state.hx")
            h0 = to_device_leaf(np.asarray(ps.hx), self.device, "real").reshape(n, L, SW).permute(1, 0, 2).contiguous()
            rs = np.asarray(requests.on_reset).reshape(-1)   # (a request built without one carries the default, one False)
            reset = to_device_leaf(np.broadcast_to(rs, (n,)) if rs.size == 1 else rs, self.device, "flag").reshape(1, n)
            ctx = RnnCtx(1, n, 1, {"a:": h0}, reset)
        hx_out = None
        self._net.begin_serving()
        self._target.begin_serving()
        try:
            adv, v = self._net.forward(obs, n, keep_tape=False, rnn=ctx)
            tadv, tv = self._target.forward(obs, n, keep_tape=False, rnn=ctx)   # (the incoming state, not the online net's new one)
            action = torch.empty((n, 1), dtype=torch.int64, device=self.device)
            value = torch.empty((n, 1), dtype=torch.float32, device=self.device)
            target_value = torch.empty((n, 1), dtype=torch.float32, device=self.device)
            hip.epsilon_greedy_sample(adv, v, tadv, tv, eps, is_eval, self.use_double_q, self._seed, self._rollout_calls, action,
                                      value, target_value)
            self._rollout_calls += 1
            out = [t.cpu().numpy() for t in (action, value, target_value)]
            if ctx is not None:
                hx_out = self._net.last_state["a:"].permute(1, 0, 2).cpu().numpy()
        finally:
            self._net.end_serving()
            self._target.end_serving()
        return policy_api.RolloutResult(action=DiscreteAction(out[0]),
                                        policy_state=DQNPolicyState(hx=hx_out, epsilon=eps_host),
                                        analyzed_result=DQNRolloutAnalyzedResult(value=out[1], target_value=out[2]))


policy_api.register("atari-dqn", AtariDQNPolicy)
