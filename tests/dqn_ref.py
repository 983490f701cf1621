"""Numpy restatement of the deep Q-learning step and of the epsilon-greedy rollout head (no GPU, no reference import).

`td_step(..., dtype=np.float64)` is the oracle: every quantity in float64, no intermediate rounding.  `dtype=np.float32` follows the
reference's own precision -- float32 network outputs, loss and statistics, float64 inside the two scalar transforms and the n-step
return with their results rounded to float32 -- so the distance between the two is "the float32 reference's own error" that the
tests' bound scales with.  tests/test_dqn_host.py pins both against the real reference's recorded outputs (tests/golden/dqn.npz).
"""
import numpy as np

from loss_ref import philox4x32_10

VALUE_LOSS = ("mse", "huber", "smoothl1")
TERMS = ("vloss", "q", "y", "qinv", "yinv", "td", "tdmax", "mask")  # the order of srl_hip.h's SRL_DQ_*


def scalar_transform(x, eps=1e-3, out=np.float32):
    """modules/utils.py:324-328: float64 arithmetic, rounded to `out`."""
    x = np.asarray(x, np.float64)
    return (np.sign(x) * (np.sqrt(np.abs(x) + 1) - 1) + eps * x).astype(out)


def inverse_scalar_transform(x, eps=1e-3, out=np.float32):
    """modules/utils.py:331-335."""
    x = np.asarray(x, np.float64)
    a = np.sqrt(1 + 4 * eps * (np.abs(x) + 1 + eps)) - 1
    return (np.sign(x) * (np.square(a / (2 * eps)) - 1)).astype(out)


def n_step_return(n, reward, nex_value, nex_done, nex_truncated, gamma, out=np.float32):
    """modules/n_step_return.py:11-50 (high_precision): leading axis time, reward / nex_* hold n + T - 1 rows."""
    reward, nex_value, nex_done, nex_truncated = (np.asarray(x, np.float64) for x in (reward, nex_value, nex_done, nex_truncated))
    T = nex_value.shape[0] - n + 1
    assert T >= 1
    ret = np.zeros_like(reward[:T])
    discount = np.ones_like(reward[:T])
    for i in range(n):
        ret += reward[i:i + T] * discount
        ret += discount * gamma * nex_truncated[i:i + T] * nex_value[i:i + T]  # truncated next: bootstrap in advance
        discount *= gamma * (1 - nex_done[i:i + T]) * (1 - nex_truncated[i:i + T])
    return (ret + discount * nex_value[n - 1:n - 1 + T]).astype(out)


def dueling_q(adv, v, dtype):
    """Q = v + adv - mean_a adv (atari_dqn_policy.py:99-101); adv [..., A], v [..., 1]."""
    adv, v = np.asarray(adv, dtype), np.asarray(v, dtype)
    return (v + adv) - adv.mean(-1, keepdims=True, dtype=dtype)


def value_loss(kind, delta, q, y):
    """l(q, y) and dl/dq of nn.MSELoss / nn.HuberLoss(delta) / nn.SmoothL1Loss(beta=delta), reduction='none', in q's dtype."""
    d = q - y
    a = np.abs(d)
    delta = d.dtype.type(delta)
    half = d.dtype.type(0.5)
    if kind == "mse":
        return d * d, 2 * d
    if kind == "huber":
        return np.where(a <= delta, half * d * d, delta * (a - half * delta)), np.where(a <= delta, d, delta * np.sign(d))
    assert kind == "smoothl1"
    return np.where(a < delta, half * d * d / delta, a - half * delta), np.where(a < delta, d / delta, np.sign(d))


def td_step(adv, v, tadv, tv, action, reward, done, truncated, weight, T, B, *, n, gamma=0.99, apply_scalar_transform=True,
            scalar_transform_eps=1e-3, double_q=True, value_loss_kind="mse", delta=1.0, eta=0.9, dtype=np.float64):
    """DeepQLearning.step between the forward passes and the backward pass (deep_q_learning.py:117-181) on the head outputs of
    AtariDQNPolicy._dqn_analyze (atari_dqn_policy.py:211-231).  Rows are time-major (row = t * B + b): adv / tadv [T*B, A], the
    rest [T*B]; weight [B] or None.  Returns a dict: d_adv [T*B, A], d_v [T*B], terms {name: float}, priorities [B], and the
    intermediate greedy [T*B], tq [T*B], q / y [S*B], loss."""
    A = adv.shape[1]
    S = T - n
    assert S >= 1
    rnd = np.float32 if dtype == np.float32 else np.float64  # where the reference rounds to float32
    q_on = dueling_q(adv, np.asarray(v).reshape(-1, 1), dtype)
    q_tg = dueling_q(tadv, np.asarray(tv).reshape(-1, 1), dtype)
    greedy = q_on.argmax(-1)  # first maximum
    rows = np.arange(T * B)
    tq = q_tg[rows, greedy] if double_q else q_tg.max(-1)
    q = q_on[rows, action][:S * B].reshape(S, B)
    tqp = inverse_scalar_transform(tq, scalar_transform_eps, rnd) if apply_scalar_transform else tq
    tqp = tqp.reshape(T, B)
    done2, trunc2 = np.asarray(done).reshape(T, B), np.asarray(truncated).reshape(T, B)
    ret = n_step_return(n, np.asarray(reward, np.float32).reshape(T, B)[:-1], tqp[1:], done2[1:], trunc2[1:], gamma, rnd)
    y = scalar_transform(ret, scalar_transform_eps, rnd) if apply_scalar_transform else ret
    mask = (1 - done2[:S]).astype(dtype)
    w = np.ones(B, dtype) if weight is None else np.asarray(weight, dtype)
    l, dl = value_loss(value_loss_kind, delta, q, y.astype(dtype))
    cnt = mask.sum(dtype=dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        loss = (l * w * mask).sum(dtype=dtype) / cnt
        g = (dl * w * mask / cnt).astype(dtype)
        td = np.abs(q - y)
        pri = dtype(eta) * (td * mask).max(0) + dtype(1 - eta) * ((td * mask).sum(0, dtype=dtype) / mask.sum(0, dtype=dtype))
    d_adv = np.zeros((T * B, A), dtype)
    onehot = (np.arange(A)[None, :] == np.asarray(action)[:S * B, None]).astype(dtype)
    d_adv[:S * B] = g.reshape(-1, 1) * (onehot - dtype(1) / dtype(A))
    d_v = np.zeros(T * B, dtype)
    d_v[:S * B] = g.reshape(-1)
    sel = mask != 0
    inv = (lambda x: inverse_scalar_transform(x, 1e-3, rnd)) if apply_scalar_transform else (lambda x: x)
    terms = dict(vloss=float((l * w * mask).sum(dtype=np.float64)), q=float(q[sel].sum(dtype=np.float64)),
                 y=float(y[sel].sum(dtype=np.float64)), qinv=float(inv(q)[sel].sum(dtype=np.float64)),
                 yinv=float(inv(y)[sel].sum(dtype=np.float64)), td=float(td[sel].sum(dtype=np.float64)),
                 tdmax=float(td[sel].max()) if sel.any() else 0.0, mask=float(cnt))
    return dict(d_adv=d_adv, d_v=d_v, terms=terms, priorities=pri, greedy=greedy, tq=tq, q=q, y=y, loss=float(loss))


def epsilon_greedy_draws(n, seed, offset, row0=0):
    """(x0, x1) of the row's Philox4x32-10 block: counter = {low, high word of row0 + row; head 0; low word of offset}, key = {low, high
    word of seed} -- the layout of the categorical sampler (loss_ref.categorical_sample)."""
    r = np.uint64(row0) + np.arange(n, dtype=np.uint64)
    m32, sh = np.uint64(0xFFFFFFFF), np.uint64(32)
    seed, offset = np.uint64(seed), np.uint64(offset)
    ctr = np.stack([r & m32, r >> sh, np.zeros(n, np.uint64), np.full(n, offset & m32)], -1)
    x = philox4x32_10(ctr, np.stack([seed & m32, seed >> sh]))
    return x[:, 0], x[:, 1]


def epsilon_greedy_sample(adv, v, tadv, tv, epsilon, is_eval, double_q, seed, offset, row0=0):
    """The rollout head (atari_dqn_policy.py:255-276) with the device's draw: u = (x0 >> 8) 2^-24; exploit iff is_eval or
    u > epsilon, else action = floor((x1 >> 8) 2^-24 A).  Q in float32 with a sequential mean, as the kernel forms it.  Returns
    action int64 [n], value and target_value float32 [n]."""
    n, A = adv.shape
    adv, tadv = np.asarray(adv, np.float32), np.asarray(tadv, np.float32)

    def q32(a, vv):
        s = np.zeros(n, np.float32)
        for j in range(A):
            s = s + a[:, j]
        return (np.asarray(vv, np.float32).reshape(n, 1) + a) - (s / np.float32(A))[:, None]

    q_on, q_tg = q32(adv, v), q32(tadv, tv)
    greedy = q_on.argmax(-1)
    x0, x1 = epsilon_greedy_draws(n, seed, offset, row0)
    u = (x0 >> np.uint64(8)).astype(np.float32) * np.float32(2.0**-24)
    rnd_action = (((x1 >> np.uint64(8)) * np.uint64(A)) >> np.uint64(24)).astype(np.int64)
    exploit = u > np.asarray(epsilon, np.float32).reshape(n)
    if is_eval is not None:
        exploit = exploit | (np.asarray(is_eval).reshape(n) != 0)
    action = np.where(exploit, greedy, rnd_action).astype(np.int64)
    rows = np.arange(n)
    return action, q_on[rows, action], (q_tg[rows, greedy] if double_q else q_tg.max(-1))


def polyak(target, param, tau, dtype=np.float64):
    """modules/utils.py:309 / :321."""
    if tau == 1:
        return np.array(param, dtype)
    return np.asarray(target, dtype) * dtype(1.0 - tau) + np.asarray(param, dtype) * dtype(tau)
