"""Inputs of the deep Q-learning kernel tests, shared between the CPU tests of the restatement (tests/test_dqn_host.py) and the device
tests (tests/test_gpu_dqn_kernels.py), and the error rule both use."""
import itertools

import numpy as np

import dqn_ref
from srl_amd.runtime import synthetic

# (T, B, A, n): S = T - n loss rows.  One loss row; a column past a wavefront; an odd A with a column past a 256-column group;
# fewer loss rows than bootstrap steps.
TD_CASES = [(2, 1, 2, 1), (8, 65, 18, 3), (9, 257, 3, 5), (4, 2, 4, 3)]
# (apply_scalar_transform, double_q, value loss, weights)
TD_VARIANTS = list(itertools.product((True, False), (True, False), dqn_ref.VALUE_LOSS, (True, False)))
DELTA = 0.75  # huber's delta / smoothl1's beta: with Q on a grid of 1/64 in [-4, 4] both branches of each loss are taken


def grid(rng, shape, top=4.0):
    """Multiples of 1/64 in [-top, top]: exact in float32, and so are v + adv and the sum over actions -- float32 and float64
    evaluations then agree on every argmax (equal Q iff equal adv), so a tie is a tie on both sides."""
    k = int(top * 64)
    return (rng.integers(-k, k + 1, size=shape) / 64.0).astype(np.float32)


def td_case(T, B, A, n, seed=0):
    """Head outputs, actions, rewards and episode flags of one case.  Flags are placed so that (where the case has the room)
      column 0 has every loss row done: its priority is 0/0;
      column 1 has `done` on the first loss row and on no other (B >= 3 and S >= 2: it would be the all-done or the last column,
      or a second all-done one, otherwise);
      the last column has `truncated` on the last bootstrapped row T - 1 and a row with both flags, and live loss rows;
      row (0, last column) holds an exact tie of its two largest online Q values.
    With B = 1 there is no all-done column: the only mask entries would all be zero and every output 0/0."""
    rng = np.random.default_rng(1000 * T + 10 * B + A + seed)
    S = T - n
    c = dict(T=T, B=B, A=A, n=n, S=S)
    for k in ("adv", "tadv"):
        c[k] = grid(rng, (T * B, A))
    for k in ("v", "tv"):
        c[k] = grid(rng, (T * B,))
    c["reward"] = grid(rng, (T * B,), top=2.0)
    c["action"] = rng.integers(0, A, size=T * B).astype(np.int32)
    done = (rng.random((T, B)) < 0.1).astype(np.uint8)
    trunc = ((rng.random((T, B)) < 0.1) & (done == 0)).astype(np.uint8)
    last = B - 1
    if last > 0:
        done[:S, last] = 0
        done[:S, 0] = 1
    else:
        done[0, 0] = 0  # keep the one column's mask non-empty
    if B >= 3 and S >= 2:
        done[:S, 1] = 0
        done[0, 1] = 1
    trunc[T - 1, last] = 1
    both = max(T - 2, 1)
    done[both, last] = trunc[both, last] = 1
    assert (done[:S, last] == 0).any()
    tie = c["adv"][last]  # row t = 0 of the last column
    tie[:] = np.minimum(tie, 1.0)
    tie[A - 1] = tie[0] = 2.0
    c["done"], c["truncated"] = done.reshape(-1), trunc.reshape(-1)
    c["weight"] = (rng.integers(16, 129, size=B) / 64.0).astype(np.float32)
    c["all_done"] = np.flatnonzero(done[:S].all(0))
    return c


def td_ref(c, variant, dtype, gamma=0.99, eta=0.9, eps=1e-3):
    ast, dq, loss, weighted = variant
    return dqn_ref.td_step(c["adv"], c["v"], c["tadv"], c["tv"], c["action"], c["reward"], c["done"], c["truncated"],
                           c["weight"] if weighted else None, c["T"], c["B"], n=c["n"], gamma=gamma, apply_scalar_transform=ast,
                           scalar_transform_eps=eps, double_q=dq, value_loss_kind=loss, delta=DELTA, eta=eta, dtype=dtype)


def assert_within(name, got, r32, r64):
    """The project's rule (tests/rnn_ref.py::check_vs_float64), per element and with none left out: |got - float64| <= 3 x |float32
    reference - float64| + 2e-6 x the tensor's largest float64 magnitude.  NaN must sit where the float64 reference has it.
    Returns the largest error / bound."""
    got, r32, r64 = (np.asarray(x, np.float64) for x in (got, r32, r64))
    nan = np.isnan(r64)
    assert np.array_equal(np.isnan(got), nan), (name, "NaN placement", np.flatnonzero(np.isnan(got) != nan)[:8])
    fin = ~nan
    top = np.abs(r64[fin]).max() if fin.any() else 0.0
    bound = 3 * np.abs(r32 - r64)[fin] + 2e-6 * top
    err = np.abs(got - r64)[fin]
    worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    assert (err <= bound).all(), (name, worst, float(err.max()), top)
    return worst


# ------------------------------------------------------------------------------------------------ end to end (tests/golden/dqn.npz)
# The fixture net: the reference's AtariDQNPolicy with hidden_dim=32, two trainer steps on two synthetic samples.
ACT, HID, CL, SEED = 6, 32, 3, 7
POLICY = dict(act_dim=ACT, dueling=True, chunk_len=CL, seed=SEED, hidden_dim=HID)
SAMPLE = dict(T=4, B=3, obs_spec={"obs": ((4, 84, 84), "u8")}, action_dims=ACT, p_done=0.15, bootstrap_steps=2)  # Tb = 6
# run -> trainer arguments.  "adam": a hard update that crosses its interval at the second step; "rmsprop": a soft update every
# step, sampling weights, huber loss, clipped gradient.  RMSprop's first steps move a weight by lr / sqrt(1 - alpha) = 10 lr:
# its lr is a tenth of Adam's, so that both move a weight by ~5e-4 per step.
RUNS = dict(
    adam=dict(bootstrap_steps=2, hard_update_interval=1, optimizer="adam", optimizer_config=dict(lr=5e-4, eps=1e-5, weight_decay=0.)),
    rmsprop=dict(bootstrap_steps=2, use_soft_update=True, tau=0.005, optimizer="rmsprop", optimizer_config=dict(lr=5e-5, eps=1e-5),
                 use_priority_weight=True, value_loss="huber", value_loss_config=dict(delta=1.0), max_grad_norm=5.0, gamma=0.97),
)
# Parameters after a step, absolute -- the bar of tests/dmlab_cases.py (PARAM_TOL there, from tests/test_gpu_smac_attn.py), derived
# the same way: 4 % of the distance one optimiser step moves a weight (5e-4 in both runs above, as in those tests).  An Adam / RMSprop
# step is lr g / (sqrt(v) + eps): where |g| is within a few eps the quotient turns float32 rounding of g into a fraction of a step.
PARAM_TOL = 2e-5
BIG = ("fc.0.weight", "fc_v.0.weight")  # the fixture keeps every STRIDE-th element of these two [32, 3136] matrices
STRIDE = 3


def e2e_arrays(step):
    """The synthetic sample of trainer step `step` (no frames in the fixture: they are drawn here) plus epsilon and the sampling
    weights."""
    arrays = synthetic.make_sample_arrays(seed=900 + step, **SAMPLE)
    rng = np.random.default_rng(77 + step)
    Tb, B = arrays["on_reset"].shape[:2]
    arrays["policy_state.epsilon"] = rng.random((Tb, B, 1)).astype(np.float32)
    arrays["sampling_weight"] = (rng.integers(32, 97, size=B) / 64.0).astype(np.float32)
    return arrays


def unpack_params(g, key, init):
    """{name: (value, encoding error, index or None)} of a state stored by gen_dqn.packq: value = init + d 2^-e."""
    out, pos = {}, 0
    for i, name in enumerate(g[key + "_names"]):
        name = str(name)
        base = np.asarray(init[name], np.float64).reshape(-1)
        idx = np.arange(0, base.size, STRIDE) if name.split(".", 1)[1] in BIG else None
        sel = base if idx is None else base[idx]
        d = g[key + "_d"][pos:pos + sel.size].astype(np.float64)
        pos += sel.size
        out[name] = (sel + d * 2.0**-int(g[key + "_e"][i]), float(g[key + "_q"][i]), idx)
    return out
