"""A torch restatement of the recurrent ``atari-dqn`` network and of ``_dqn_analyze`` (reference
``q_learning/game_policies/atari_dqn_policy.py:29-101,168-236``), with one difference: the towers read ``hidden_dim`` columns, not
512, so it also runs at the small widths the chunk kernels are tested at.  At ``hidden_dim=512`` it IS the reference's network,
and tests/test_r2d2_host.py holds it to the reference's recorded run (tests/golden/r2d2.npz) there before anything else trusts it.

The ``state_dict`` keys are the reference's.  It runs in float32 or float64; the device tests take the float64 run as the oracle and
the float32 run as the measure of what float32 arithmetic costs (``rnn_ref.check_vs_float64``).
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F


class AutoResetRNN(nn.Module):
    """nn.GRU / nn.LSTM whose state is multiplied by ``1 - on_reset[t]`` in front of every step; an LSTM's state is ``cat(h, c)``."""

    def __init__(self, input_dim, hidden, layers, kind):
        super().__init__()
        self.kind = kind
        self.__net = (nn.LSTM if kind == "lstm" else nn.GRU)(input_dim, hidden, num_layers=layers)

    def forward(self, x, h, on_reset):
        ys = []
        for t in range(x.shape[0]):
            h = h * (1 - on_reset[t]).view(1, -1, 1)
            if self.kind == "lstm":
                y, (a, b) = self.__net(x[t:t + 1], tuple(s.contiguous() for s in h.chunk(2, -1)))
                h = torch.cat([a, b], -1)
            else:
                y, h = self.__net(x[t:t + 1], h)
            ys.append(y)
        return torch.cat(ys, 0), h


class Net(nn.Module):

    def __init__(self, act_dim, hidden_dim, num_rnn_layers, rnn_type):
        super().__init__()
        self.conv1, self.conv2, self.conv3 = nn.Conv2d(4, 32, 8, 4), nn.Conv2d(32, 64, 4, 2), nn.Conv2d(64, 64, 3, 1)
        self.rnn = AutoResetRNN(3136, hidden_dim, num_rnn_layers, rnn_type)
        self.fc = nn.Sequential(nn.Linear(hidden_dim, hidden_dim), nn.ReLU(), nn.Linear(hidden_dim, act_dim))
        self.fc_v = nn.Sequential(nn.Linear(hidden_dim, hidden_dim), nn.ReLU(), nn.Linear(hidden_dim, 1))

    def forward(self, frames, hx, on_reset):
        """frames [T, N, 4, 84, 84] / 255 already; hx [layers, N, SW]; on_reset [T, N, 1].  Returns (adv [T, N, A], v [T, N, 1], hx')."""
        T, N = frames.shape[:2]
        x = frames.reshape(T * N, 4, 84, 84)
        for conv in (self.conv1, self.conv2, self.conv3):
            x = F.relu(conv(x))
        x, hx = self.rnn(x.reshape(T, N, -1), hx, on_reset)
        return self.fc(x), self.fc_v(x), hx


def make_net(state, prefix, policy, dtype):
    """``Net`` with the parameters ``<prefix><name>`` of ``state`` (numpy, the reference's keys) in ``dtype``."""
    net = Net(policy["act_dim"], policy["hidden_dim"], policy["num_rnn_layers"], policy["rnn_type"]).to(dtype)
    net.load_state_dict({k[len(prefix):]: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in state.items() if k.startswith(prefix)})
    return net


def to_chunk(x, k):
    return torch.cat(torch.split(x, x.shape[0] // k, dim=0), dim=1)


def from_chunk(x, k):
    return torch.cat(torch.split(x, x.shape[1] // k, dim=1), dim=0)


def burn_in_windows(rows, burn, chunk_len):
    """The literal indices of :169-183: (num_chunks, [(start, stop) of each chunk's burn-in rows in the full sample])."""
    num_chunks = (rows - burn) // chunk_len
    return num_chunks, [(i * chunk_len, i * chunk_len + burn) for i in range(num_chunks)]


def analyze(net, target, arrays, burn, chunk_len, dtype):
    """``arrays``: the flat sample (``obs.obs`` uint8 [Tb, B, 4, 84, 84], ``policy_state.hx`` [Tb, B, layers, SW], ``on_reset``,
    ``action.x``).  Returns head outputs of both networks for rows [burn, Tb) as trajectories, ``adv [T, B, A]``, ``v [T, B, 1]``
    (online, with autograd), ``tadv``, ``tv``, and the reference's ``q_tot`` / ``target_q_tot`` [T, B, 1]."""
    t = lambda k: torch.as_tensor(arrays[k]).to(dtype)
    frames, hx_all, on_reset, action = t("obs.obs") / 255.0, t("policy_state.hx"), t("on_reset"), torch.as_tensor(arrays["action.x"]).long()
    K, windows = burn_in_windows(frames.shape[0], burn, chunk_len)
    ck = lambda x: to_chunk(x[burn:], K)
    if burn == 0:
        hx = ck(hx_all)[0].transpose(0, 1)
    else:
        cat = lambda x: torch.cat([x[a:b] for a, b in windows], dim=1)
        with torch.no_grad():
            _, _, hx = net(cat(frames), cat(hx_all)[0].transpose(0, 1), cat(on_reset))
    adv, v, _ = net(ck(frames), hx, ck(on_reset))
    with torch.no_grad():
        tadv, tv, _ = target(ck(frames), hx, ck(on_reset))
    qf, tqf = v + adv - adv.mean(-1, keepdim=True), tv + tadv - tadv.mean(-1, keepdim=True)
    q_tot = qf.gather(-1, ck(action))
    target_q_tot = tqf.gather(-1, qf.argmax(-1, keepdim=True))
    out = dict(adv=adv, v=v, tadv=tadv, tv=tv, q_tot=q_tot, target_q_tot=target_q_tot)
    return {k: from_chunk(x, K) for k, x in out.items()}
