"""``dmlab``: IMPALA's DMLab-30 agent on the HIP kernels.

Mirror of ``DMLabActorCriticPolicy`` (reference ``legacy/algorithm/ppo/game_policies/dmlab_policy.py:171-367``): the same
constructor keywords and defaults, the same ``state_dict`` names, ``analyze(target="ppo", burn_in_steps=...)`` and ``rollout``.
The network (``netspec.build_dmlab_netspec``) has two encoders -- the pixels ``obs`` (``/ 255``, two strided convolutions, a
Linear; no LayerNorm anywhere) and the instruction ``INSTR`` (token ids ``[.., L]``: a word embedding and a length-masked LSTM, one
HIP launch per direction, ``csrc/instr_lstm.hip``) -- whose concatenation feeds one shared ``AutoResetRNN``; the actor and the
(PopArt) critic head read its output.

``INSTR`` may come in any integer or float dtype (a float is truncated towards zero like the reference's ``.long()``); it travels as
float32, or as int32 when it already is.  DIFFERENCE: a token outside ``[0, 1000)`` is treated as padding where the reference's
``nn.Embedding`` raises.  ``num_dense_layers > 0``, ``rnn_type="gtrxl"`` and sizes the fused language encoder does not take
(``hip.instr_lstm_supported``) raise ``NotImplementedError`` at construction.
"""
import numpy as np

from srl_amd import hip
from srl_amd.algorithm import netspec as ns
from srl_amd.algorithm.actor_critic import ActorCriticPolicy
from srl_amd.api import policy as policy_api
from srl_amd.namedarray import NamedArray

DMLAB_INSTRUCTIONS = "INSTR"


class DMLabPolicy(ActorCriticPolicy):

    def __init__(self,
                 obs_shapes,
                 action_dim: int,
                 hidden_dim: int = 512,
                 chunk_len: int = 10,
                 num_dense_layers: int = 0,
                 rnn_type: str = "lstm",
                 num_rnn_layers: int = 1,
                 popart: bool = True,
                 activation: str = "relu",
                 layernorm: bool = False,
                 seed=0,
                 popart_beta: float = 0.99999,
                 **kwargs):
        policy_api.Policy.__init__(self)
        self.spec, init = ns.build_dmlab_netspec(obs_shapes, int(action_dim), hidden_dim, num_dense_layers=num_dense_layers,
                                                 rnn_type=rnn_type, num_rnn_layers=num_rnn_layers, popart=popart,
                                                 activation=activation, layernorm=layernorm, seed=seed, **kwargs)
        A = self.spec.obs_encoders[1].layers[0]
        if not hip.instr_lstm_supported(A.vocab, A.embed, A.units, A.length):
            raise NotImplementedError(
                f"dmlab: the fused language encoder takes up to 65536 words of at most 32 columns, 32 or 64 LSTM units and 1 to 64 "
                f"tokens per row; got {A.vocab} words of {A.embed}, {A.units} units, INSTR {(A.length,)}")
        self._setup(init, chunk_len, seed)
        self._popart_beta = float(popart_beta)   # reaches PopArt's update (ActorCriticPolicy.update_popart_from_stats)

    def _rollout(self, requests: policy_api.RolloutRequest, **kwargs):
        # the reference hands `on_reset` to the network with the carried state (:326-331): AutoResetRNN starts an episode's first
        # step from zeros (autoreset_rnn.py:46-59), where the generic policy uses the state as given
        ps = requests.policy_state
        if self.spec.num_rnn_layers and ps is not None:
            hx = np.asarray(ps["hx"], dtype=np.float32)
            keep = 1.0 - np.asarray(requests.on_reset, dtype=np.float32).reshape(hx.shape[0], 1, 1)
            requests = policy_api.RolloutRequest(obs=requests.obs, policy_state=NamedArray(hx=hx * keep),
                                                 is_evaluation=requests.is_evaluation, on_reset=requests.on_reset)
        return super()._rollout(requests, **kwargs)


policy_api.register("dmlab", DMLabPolicy)
