"""The recurrent ``atari-dqn`` (R2D2) cases shared between the fixture's generator (tests/golden/gen_r2d2.py), the CPU tests
(tests/test_r2d2_host.py) and the device tests (tests/test_gpu_r2d2.py).

Two recorded runs of the REAL reference at ``hidden_dim=512`` (the only width at which its recurrent agent runs: its towers read
512 columns whatever ``hidden_dim`` is), two ``DeepQLearning.step`` calls each, trainer arguments those of ``dqn_cases.RUNS``:
  gru   one GRU layer, chunk_len 4, burn_in_steps 2, Tb = 10: two chunks of 4, each burn-in window directly in front of its chunk;
  lstm  two LSTM layers, chunk_len 3, no burn-in, Tb = 8: 8 // 3 = two chunks of 4 (C != chunk_len); RMSprop, soft update,
        sampling weights, huber loss, clipped norm.

Bars: the project's -- 1e-5 relative on analyze outputs, statistics and priorities (``close``), ``dqn_cases.PARAM_TOL`` less the
fixture's encoding error on parameters.  The generator also runs every case in float64 and records, per compared quantity, the
distance of the reference's OWN float32 run from its float64 run in units of that bar (``<run>_f64_<quantity>``).  Where that
distance exceeds a third of the bar, float32 arithmetic in another order cannot be expected inside it, and the quantity's bar becomes
three times the recorded distance (``bar_scale``); everywhere else the bar stays as it is.  The measure is the reference alone,
never this project's output.
"""
import numpy as np

import dqn_cases
from srl_amd.runtime import synthetic

ACT, B, HID = 6, 3, 512
RUNS = dict(
    gru=dict(policy=dict(act_dim=ACT, dueling=True, chunk_len=4, seed=11, hidden_dim=HID, num_rnn_layers=1, rnn_type="gru"),
             trainer=dict(dqn_cases.RUNS["adam"], burn_in_steps=2), Tb=10, sample_seed=350),
    lstm=dict(policy=dict(act_dim=ACT, dueling=True, chunk_len=3, seed=11, hidden_dim=HID, num_rnn_layers=2, rnn_type="lstm"),
              trainer=dict(dqn_cases.RUNS["rmsprop"]), Tb=8, sample_seed=300),
)
TABLES = dict(gru1=RUNS["gru"]["policy"], lstm2=RUNS["lstm"]["policy"])
TABLE_STRIDE = 997
PARAM_TOL = dqn_cases.PARAM_TOL
QUANTITIES = ("q_tot", "target_q_tot", "stats0", "stats1", "priorities0", "priorities1", "params")


def state_width(policy):
    return policy["hidden_dim"] * (2 if policy["rnn_type"] == "lstm" else 1)


def e2e_arrays(run, step):
    """The synthetic sample of trainer step ``step`` of ``run``: frames, flags, actions and rewards of ``make_sample_arrays``, a seeded
    stored state ``policy_state.hx`` of 0.3 N(0, 1), epsilon and the sampling weights."""
    r = RUNS[run]
    arrays = synthetic.make_sample_arrays(seed=r["sample_seed"] + step, T=r["Tb"] - 2, B=B, obs_spec={"obs": ((4, 84, 84), "u8")},
                                          action_dims=ACT, p_done=0.2, bootstrap_steps=2)
    rng = np.random.default_rng(r["sample_seed"] + 50 + step)
    Tb = arrays["on_reset"].shape[0]
    L, SW = r["policy"]["num_rnn_layers"], state_width(r["policy"])
    arrays["policy_state.hx"] = (0.3 * rng.standard_normal((Tb, B, L, SW))).astype(np.float32)
    arrays["policy_state.epsilon"] = rng.random((Tb, B, 1)).astype(np.float32)
    arrays["sampling_weight"] = (rng.integers(32, 97, size=B) / 64.0).astype(np.float32)
    return arrays


def stride_of(numel):
    """Every ``stride``-th element of a tensor is kept in the fixture: at most ~4096 per tensor, an odd stride so that the kept
    elements walk through rows and columns alike."""
    return max(1, numel // 4096) | 1


def unpack_params(g, key, init):
    """{name: (value, encoding error, index)} of a state stored by gen_r2d2.packq: value = init + d 2^-e on every stride-th element."""
    out, pos = {}, 0
    for i, name in enumerate(g[key + "_names"]):
        name = str(name)
        base = np.asarray(init[name], np.float64).reshape(-1)
        idx = np.arange(0, base.size, stride_of(base.size))
        d = g[key + "_d"][pos:pos + idx.size].astype(np.float64)
        pos += idx.size
        out[name] = (base[idx] + d * 2.0**-int(g[key + "_e"][i]), float(g[key + "_q"][i]), idx)
    return out


def bar_scale(g, run, quantity):
    """1, or three times the reference's own float32-to-float64 distance (in units of the bar) where that exceeds a third."""
    dist = float(g[f"{run}_f64_{quantity}"])
    return 3.0 * dist if dist > 1.0 / 3.0 else 1.0


def rel_err(got, want, floor):
    """Largest |got - want| in units of max(|want|, floor): ``close`` of tests/test_gpu_dqn.py holds it to 1e-5."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float((np.abs(got - want) / np.maximum(np.abs(want), floor)).max())
