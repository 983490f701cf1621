"""Plain restatements of the discrete-action heads, their Philox sampler, the PPO loss and the masked normalisation, on the CPU
(torch with autograd / numpy), buffer by buffer as the HIP kernels see them (csrc/categorical.hip: `srl_categorical_fwd / _bwd /
_sample`; csrc/ppo_loss.hip: `srl_ppo_loss_fwd_bwd`; csrc/gae.hip: `srl_masked_stats / _normalize`; the head normalisation, the
Philox draw and the value loss are stated once on the device, in csrc/action_dist.h).  No GPU and no project code.

Run in float64 they are the reference the kernels are held to (tests/test_gpu_loss_kernels.py); run in float32 they measure how far
an honest float32 evaluation of the same arithmetic lands from float64, which sets the tolerance.  tests/test_loss_reference.py
holds them against finite differences, Philox's known answers and the float32 oracle (oracle/ppo.py).

Every result comes with an *error scale*: the sum of the magnitudes of the terms it is a sum of, from the float64 run alone; a float32
evaluation is off by a few 2^-24 of it.  Where a term passes through exp, the absolute error of the exponent is the relative error
of the term, so such a term is weighted by 1 + the magnitudes the exponent is a sum of (`cond` below).

`FAULTS` are deliberate errors of these restatements, used only to show that the tolerances can fail.  The second half of the file
holds the inputs of the GPU tests and the comparisons both test files apply, so that the CPU tests judge the very inputs and bounds
the kernels are judged by."""
import functools

import numpy as np
import torch

CAT_FAULTS = ("entropy_grad_sign", "masked_gets_gradient")
SAMPLE_FAULTS = ("heads_share_draw", "row0_ignored", "picks_unavailable")
LOSS_FAULTS = ("mean_over_channels", "mask_not_inverted", "huber_linear_slope", "dual_clip_off", "norm_by_local_n")
FAULTS = CAT_FAULTS + SAMPLE_FAULTS + LOSS_FAULTS

MASKED_LOGIT = -1e10  # actor_critic_policy.py:136
LOSS_TERMS = ("policy", "value", "entropy", "clip", "ratio", "adv", "ret", "mask", "done", "trunc")  # srl_hip.h: SRL_LT_*
NEAR = 1e-5  # an element within this (relative) of a branch point is *near a branch*: float32 may land on the other side


def _f32(x):
    """A hyper-parameter as the kernel holds it: a C float."""
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------------ categorical heads
def _heads(dims):
    s = 0
    for k, d in enumerate(dims):
        yield k, s, d
        s += d


def _masked(logits, avail):
    z = np.asarray(logits, np.float64).copy()
    if avail is not None:
        z[np.asarray(avail) == 0] = MASKED_LOGIT
    return z


def categorical(logits, action, avail, dims, d_logp=None, d_ent=None, dtype=torch.float64, fault=None):
    """torch.distributions.Categorical per head on masked_fill(avail == 0, -1e10) (actor_critic_policy.py:135-136, 311-324), in
    ``dtype``.  logits float32 [n, sum(dims)], action integer [n, heads], avail uint8 [n, sum(dims)] or None, d_logp / d_ent float32
    [n] (None: forward only).  Returns (out, scales), float64 numpy:
      out     logp, ent [n]: the sums over the LIVE heads; d_logits [n, sum(dims)] = d (sum logp d_logp + ent d_ent) / d logits;
              dead [n, heads]: no action of the head is available (a dead agent); logp_dead, ent_dead [n]: what the dead heads
              would add in exact arithmetic, -log d and log d each (uniform over the head's d actions) -- and do NOT add in
              float32, the arithmetic of the reference project and of the kernels: every masked logit is -1e10, where float32 is
              spaced 1024 apart, so logsumexp = fl(-1e10 + log d) = -1e10, every normalised logit is -1e10 - (-1e10) = 0 exactly,
              the log-prob is 0 and the entropy -sum p 0 = 0.  float32 torch.distributions.Categorical gives these zeros
              (tests/test_loss_reference.py asserts it) and csrc/action_dist.h's head_norm, the one normalisation every categorical
              kernel calls, computes lse = mx + logf(se) the same way, so a dead
              head's share is pinned to exactly 0 and logp / ent are held to the live heads' sum at the live heads' scale.
      scales  logp, ent [n], d_logits [n, sum(dims)]: the error scales (module docstring) of the live heads (0 where every head is
              dead); d_logits has scale 0, and must be exactly 0, at unavailable actions and in dead heads.  With z the masked
              logits, nl = z - max - log se = log p, H the head's entropy and cond_j = 1 + |z_j| + |max| + |log se| (what the absolute
              error of nl_j, the relative error of p_j, is made of):  logp: cond at the action;  ent: sum_j p_j (1 + |nl_j|) cond_j;
              d_logits_j: (|d_logp| (1[j = a] + p_j) + |d_ent| p_j (1 + |nl_j| + H)) cond_j -- the 1 beside |nl_j| + H because that
              sum carries nl_j's absolute error however small it is itself; and p_j no smaller than 2^-102 there: below
              float32's smallest normal number, 2^-126, p_j is denormal or flushed to 0: an absolute error of up to 2^-126 =
              2^-24 2^-102."""
    lg = torch.from_numpy(np.ascontiguousarray(logits)).to(dtype).requires_grad_(d_logp is not None)
    act = torch.from_numpy(np.ascontiguousarray(action)).long()
    x = lg
    if avail is not None:
        off = torch.from_numpy(np.ascontiguousarray(avail)) == 0
        if fault == "masked_gets_gradient":  # the value is overwritten, the gradient still flows
            x = torch.where(off, lg - lg.detach() + MASKED_LOGIT, lg)
        else:
            x = lg.masked_fill(off, MASKED_LOGIT)
    lp, ent = 0, 0
    for k, s, d in _heads(dims):
        dist = torch.distributions.Categorical(logits=x[:, s:s + d])
        lpk, hk = dist.log_prob(act[:, k]), dist.entropy()
        if avail is not None:  # a dead head adds exactly 0 (docstring); under the fault its gradient still flows
            live = ~off[:, s:s + d].all(1)
            zero = (lambda t: t - t.detach()) if fault == "masked_gets_gradient" else torch.zeros_like
            lpk, hk = torch.where(live, lpk, zero(lpk)), torch.where(live, hk, zero(hk))
        lp = lp + lpk
        ent = ent + hk
    out = dict(logp=lp.detach().double().numpy(), ent=ent.detach().double().numpy())
    if d_logp is not None:
        g_ent = torch.from_numpy(d_ent).to(dtype) * (-1 if fault == "entropy_grad_sign" else 1)
        (lp * torch.from_numpy(d_logp).to(dtype) + ent * g_ent).sum().backward()
        out["d_logits"] = lg.grad.double().numpy()

    # error scales, float64 numpy, from the inputs alone
    n = logits.shape[0]
    z = _masked(logits, avail)
    on = np.ones(z.shape, bool) if avail is None else np.asarray(avail) != 0
    gl = np.zeros(n) if d_logp is None else np.abs(d_logp.astype(np.float64))
    ge = np.zeros(n) if d_ent is None else np.abs(d_ent.astype(np.float64))
    sc = dict(logp=np.zeros(n), ent=np.zeros(n), d_logits=np.zeros(z.shape))
    dead = np.zeros((n, len(dims)), bool)
    out["logp_dead"], out["ent_dead"] = np.zeros(n), np.zeros(n)
    rows = np.arange(n)
    for k, s, d in _heads(dims):
        zk, onk = z[:, s:s + d], on[:, s:s + d]
        live = onk.any(1)
        dead[:, k] = ~live
        mx = zk.max(1)
        se = np.exp(zk - mx[:, None]).sum(1)
        nl = zk - (mx + np.log(se))[:, None]
        p = np.exp(nl)
        hk = -(p * nl).sum(1)
        cond = np.where(onk, 1.0 + np.abs(zk) + (np.abs(mx) + np.abs(np.log(se)))[:, None], 0.0)
        a = np.asarray(action)[:, k].astype(np.int64)
        taken = np.zeros((n, d))
        taken[rows, a] = 1.0
        logd = np.log(float(d))
        sc["logp"] += np.where(live, cond[rows, a], 0.0)
        sc["ent"] += np.where(live, (p * (1.0 + np.abs(nl)) * cond).sum(1), 0.0)
        pf = np.maximum(p, 2.0**-102)  # float32 holds no p below 2^-126 (2^-102 in units of 2^-24) relatively: the error is absolute
        g_mag = gl[:, None] * (taken + pf) + ge[:, None] * pf * (1.0 + np.abs(nl) + hk[:, None])
        sc["d_logits"][:, s:s + d] = np.where(live[:, None] & onk, g_mag * cond, 0.0)
        out["logp_dead"] -= np.where(live, 0.0, logd)
        out["ent_dead"] += np.where(live, 0.0, logd)
    out["dead"] = dead
    return out, sc


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al. 2011, "Parallel random numbers: as easy as 1, 2, 3") in numpy uint64: counter [..., 4] and key
    [..., 2] hold 32-bit words; returns the four 32-bit output words [..., 4] as uint64."""
    m32 = np.uint64(0xFFFFFFFF)
    M0, M1, W0, W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    c = [np.asarray(counter, np.uint64)[..., i] & m32 for i in range(4)]
    k = [np.asarray(key, np.uint64)[..., i] & m32 for i in range(2)]
    sh = np.uint64(32)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]  # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> sh) ^ c[1] ^ k[0], p1 & m32, (p0 >> sh) ^ c[3] ^ k[1], p0 & m32]
        k = [(k[0] + W0) & m32, (k[1] + W1) & m32]
    return np.stack(np.broadcast_arrays(*c), -1)


def categorical_sample(logits, avail, is_eval, dims, seed, offset, row0=0, fault=None):
    """The rollout's inverse-CDF sampler in float64.  Per (row, head): counter = {(row0 + row) & 0xffffffff, (row0 + row) >> 32, head,
    offset & 0xffffffff}, key = {seed & 0xffffffff, seed >> 32}; with x the first output word, e_j = exp(z_j - max z) over the masked
    logits and se their sum, u = (x >> 8) 2^-24 se and the pick is the first j with u < e_0 + ... + e_j.  A row with is_eval picks the
    first maximum of the masked logits.  Returns action int64 [n, heads], u and se [n, heads] and
      ambiguous [n, heads]: |u - cdf_j| <= (d + 4) 2^-23 se for an inner boundary j < d - 1.  A float32 evaluation reaches cdf_j by at
      most d additions of terms bounded by se (2^-24 se each), the terms come from an expf good to two ulp (sum e_j 2^-23 <= 2^-23
      se), and u is a rounded product (2^-24 se) with a float32 se (d + 2 roundings more on its own): inside the band it may pick
      j + 1 for j or the reverse, outside it it may not."""
    n = logits.shape[0]
    z = _masked(logits, None if fault == "picks_unavailable" else avail)
    r = (np.uint64(0) if fault == "row0_ignored" else np.uint64(row0)) + np.arange(n, dtype=np.uint64)
    m32, sh = np.uint64(0xFFFFFFFF), np.uint64(32)
    seed, offset = np.uint64(seed), np.uint64(offset)
    key = np.stack([seed & m32, seed >> sh])
    action = np.zeros((n, len(dims)), np.int64)
    amb = np.zeros((n, len(dims)), bool)
    us, ses = np.zeros((n, len(dims))), np.zeros((n, len(dims)))
    greedy = np.zeros(n, bool) if is_eval is None else np.asarray(is_eval) != 0
    for k, s, d in _heads(dims):
        zk = z[:, s:s + d]
        mx = zk.max(1)
        e = np.exp(zk - mx[:, None])
        cdf = np.cumsum(e, 1)
        se = cdf[:, -1]
        head = np.uint64(0 if fault == "heads_share_draw" else k)
        ctr = np.stack([r & m32, r >> sh, np.broadcast_to(head, r.shape), np.broadcast_to(offset & m32, r.shape)], -1)
        x = philox4x32_10(ctr, key)[:, 0]
        u = (x >> np.uint64(8)).astype(np.float64) * 2.0**-24 * se
        pick = (u[:, None] >= cdf).sum(1)  # the first j with u < cdf_j (u < se = cdf_{d-1} always)
        action[:, k] = np.where(greedy, zk.argmax(1), np.minimum(pick, d - 1))
        amb[:, k] = ~greedy & (np.abs(u[:, None] - cdf[:, :d - 1]) <= (d + 4) * 2.0**-23 * se[:, None]).any(1)
        us[:, k], ses[:, k] = u, se
    return dict(action=action, ambiguous=amb, u=us, se=ses)


# ------------------------------------------------------------------------------------------------ PPO loss
def _value_loss(kind, delta, v, t, fault=None):
    """modules/utils.py:228-265: nn.MSELoss / nn.HuberLoss(delta) / nn.SmoothL1Loss(beta = delta), reduction 'none'."""
    d = v - t
    if kind == "mse":
        return d * d
    a = d.abs()
    quad, lin = (0.5 * d * d, delta * (a - 0.5 * delta)) if kind == "huber" else (0.5 * d * d / delta, a - 0.5 * delta)
    if fault == "huber_linear_slope":  # the right value, the quadratic's slope past delta
        lin = lin.detach() + quad - quad.detach()
    return torch.where(a <= delta, quad, lin) if kind == "huber" else torch.where(a < delta, quad, lin)


def ppo_loss(inputs, hp, norm_stats, local_n, mask_invert, dtype=torch.float64, fault=None):
    """MultiAgentPPO._compute_loss (mappo.py:146-217) and its backward as `srl_ppo_loss_fwd_bwd` states them (srl_hip.h).
    inputs: new_lp, old_lp, entropy float32 [n]; value, old_value, adv, ret float32 [n, vd]; mask uint8 [n], the byte as the kernel
    gets it (mask_invert: the mask is 1 - byte); done, truncated uint8 [n] or absent.  hp: eps_clip, c_clip, value_eps_clip,
    value_loss_weight, entropy_bonus_weight, huber_delta, norm_eps (used as C floats), dual_clip, clip_value, value_loss
    ("mse" / "huber" / "smoothl1").  norm_stats (n, s, q): the global sums of the advantage normalisation; local_n: this rank's mask sum.
      nadv = float32(((adv m) - s/n) / (sqrt(q/n - (s/n)^2) + norm_eps)), in float64 and rounded once (utils.py:62-67), [n, vd]
      ratio = exp(new_lp - old_lp); s1 = ratio nadv; s2 = clamp(ratio, 1 -+ eps_clip) nadv; s3 = -c_clip |nadv|
      policy = -max(min(s1, s2), s3) (dual clip) or -min(s1, s2); value = l(v, ret) or max(l(v, ret), l(old + clamp(v - old), ret))
      loss = (sum m policy + w_v sum m value - w_H sum m entropy) / local_n: m, ratio and entropy broadcast over the vd channels,
      every sum runs over all channels and divides by the count of ROWS (mappo.py:184,197)
    Returns a dict of float64 numpy: d_new_lp, d_entropy [n], d_value [n, vd]; terms: the ten masked sums by LOSS_TERMS name; and,
    from a float64 run only: scales (per element, keys as the gradients), term_mag (per term: the sum of the magnitudes of its
    terms), elem_mag (policy, value [n, vd]: what term_mag sums), near_p / near_v [n, vd]: the element lies within NEAR (relative) of
    a branch point of the policy term (either ratio clip; s1 = s2 outside the clip range, which is nadv = 0; min(s1, s2) = s3) or of
    the value term (|v - ret| = delta for v or the clipped v; |v - old| = value_eps_clip; l1 = l2 with v != clipped v)."""
    t = lambda k: torch.from_numpy(np.ascontiguousarray(inputs[k])).to(dtype)
    byte = np.asarray(inputs["mask"]).astype(np.float64)
    m64 = 1.0 - byte if (mask_invert and fault != "mask_not_inverted") else byte
    n, vd = inputs["value"].shape
    cnt, s, q = (float(v) for v in norm_stats)
    local_n = float(local_n)
    if fault == "norm_by_local_n":
        cnt = local_n
    mean = s / cnt
    with np.errstate(invalid="ignore"):  # statistics that are no one's (a fault's) may hold a negative variance: NaN, as on the device
        denom = np.sqrt(q / cnt - mean * mean) + _f32(hp["norm_eps"])
    adv64 = inputs["adv"].astype(np.float64)
    nadv = torch.from_numpy((((adv64 * m64[:, None]) - mean) / denom).astype(np.float32)).to(dtype)
    m = torch.from_numpy(m64).to(dtype)[:, None]
    eps, c_clip, veps, delta = _f32(hp["eps_clip"]), _f32(hp["c_clip"]), _f32(hp["value_eps_clip"]), _f32(hp["huber_delta"])
    w_v, w_h = _f32(hp["value_loss_weight"]), _f32(hp["entropy_bonus_weight"])
    kind = hp["value_loss"]
    new_lp, v, ent = t("new_lp").requires_grad_(True), t("value").requires_grad_(True), t("entropy").requires_grad_(True)
    ratio = (new_lp - t("old_lp")).exp()[:, None]
    s1 = ratio * nadv
    s2 = ratio.clamp(1.0 - eps, 1.0 + eps) * nadv
    mn = torch.min(s1, s2)
    dual = bool(hp["dual_clip"]) and fault != "dual_clip_off"
    s3 = -torch.sign(nadv) * c_clip * nadv
    pl = -torch.max(mn, s3) if dual else -mn
    ret = t("ret")
    l1 = _value_loss(kind, delta, v, ret, fault)
    vl = l1
    if hp["clip_value"]:
        vo = t("old_value")
        vc = vo + (v - vo).clamp(-veps, veps)
        l2 = _value_loss(kind, delta, vc, ret, fault)
        vl = torch.max(l1, l2)
    per_row = local_n * (vd if fault == "mean_over_channels" else 1)
    loss = (pl * m).sum() / per_row + w_v * (vl * m).sum() / per_row - w_h * (ent * m[:, 0]).sum() / local_n
    loss.backward()
    np64 = lambda x: x.detach().double().numpy()
    res = dict(d_new_lp=np64(new_lp.grad), d_value=np64(v.grad), d_entropy=np64(ent.grad))
    pl64, vl64, ratio64, s1_64, s2_64 = np64(pl), np64(vl), np64(ratio), np64(s1), np64(s2)
    ret64 = inputs["ret"].astype(np.float64)
    count = lambda k: float(np.asarray(inputs[k]).astype(np.float64).sum()) if inputs.get(k) is not None else 0.0
    res["terms"] = dict(policy=(m64[:, None] * pl64).sum(), value=(m64[:, None] * vl64).sum(), entropy=(m64 * np64(ent)).sum(),
                        clip=(m64[:, None] * (s2_64 < s1_64)).sum(), ratio=(m64 * ratio64[:, 0]).sum(), adv=(m64[:, None] * adv64).sum(),
                        ret=(m64[:, None] * ret64).sum(), mask=m64.sum(),
                        done=count("done"), trunc=count("truncated"))
    res["sign_terms"] = dict(adv=(m64[:, None] * np.abs(adv64)).sum(), ret=(m64[:, None] * np.abs(ret64)).sum())
    if dtype != torch.float64:
        return res

    # error scales and branch flags, from the float64 values
    w = m64 / local_n
    nadv64, v64, mn64, s3_64 = np64(nadv), np64(v), np64(mn), np64(s3)
    lo, hi = 1.0 - eps, 1.0 + eps
    near_p = (np.abs(ratio64 - lo) <= NEAR * lo) | (np.abs(ratio64 - hi) <= NEAR * hi) | (nadv64 == 0.0)
    near_p = np.broadcast_to(near_p, (n, vd)).copy()
    if dual:
        near_p |= np.abs(mn64 - s3_64) <= NEAR * np.maximum(np.abs(mn64), np.abs(s3_64))
    mag_in = np.abs(v64) + np.abs(ret64)  # what v - ret is a difference of
    d1 = np.abs(v64 - ret64)
    near_v = np.zeros((n, vd), bool)
    if kind != "mse":
        near_v |= np.abs(d1 - delta) <= NEAR * delta
    lin = d1 > delta if kind == "huber" else d1 >= delta  # the branch of the loss that wins
    if hp["clip_value"]:
        vo64, vc64, l1_64, l2_64 = np64(vo), np64(vc), np64(l1), np64(l2)
        mag_in = mag_in + 2.0 * np.abs(vo64)  # vc = old + (v - old)
        d2 = np.abs(vc64 - ret64)
        near_v |= np.abs(np.abs(v64 - vo64) - veps) <= NEAR * veps
        near_v |= (v64 != vc64) & (np.abs(l1_64 - l2_64) <= NEAR * np.maximum(l1_64, l2_64))
        if kind != "mse":
            near_v |= np.abs(d2 - delta) <= NEAR * delta
        lin = np.where(l1_64 >= l2_64, lin, d2 > delta if kind == "huber" else d2 >= delta)
    if kind == "mse":
        slope, vmag = 2.0 * mag_in, mag_in * mag_in
    elif kind == "huber":
        slope, vmag = np.where(lin, delta, mag_in), np.where(lin, delta * (mag_in + 0.5 * delta), 0.5 * mag_in * mag_in)
    else:
        slope, vmag = np.where(lin, 1.0, mag_in / delta), np.where(lin, mag_in + 0.5 * delta, 0.5 * mag_in * mag_in / delta)
    res["scales"] = dict(d_new_lp=(np.abs(nadv64) * ratio64).sum(1) * w, d_value=w_v * slope * w[:, None], d_entropy=w_h * w)
    res["elem_mag"] = dict(policy=np.abs(pl64), value=vmag)
    res["term_mag"] = dict(policy=(m64[:, None] * np.abs(pl64)).sum(), value=(m64[:, None] * vmag).sum(),
                           entropy=(m64 * np.abs(np64(ent))).sum(), ratio=(m64 * ratio64[:, 0]).sum())
    res["near_p"], res["near_v"], res["m"], res["clip_elem"] = near_p, near_v, m64, s2_64 < s1_64
    res["branches"] = dict(below=ratio64[:, 0] < lo, above=ratio64[:, 0] > hi, dual=(mn64 < s3_64) if dual else np.zeros((n, vd), bool),
                           linear=lin if kind != "mse" else np.zeros((n, vd), bool))
    if hp["clip_value"]:
        clipped = np.abs(v64 - vo64) > veps
        res["branches"].update(vclip_l1=clipped & (l1_64 > l2_64), vclip_l2=clipped & (l2_64 > l1_64))
    return res


# ------------------------------------------------------------------------------------------------ masked normalisation
def masked_stats(x, mask=None, mask_invert=False):
    """(count, sum x m, sum (x m)^2) in float64 and the sums of the terms' magnitudes (utils.py:38-57)."""
    x = np.asarray(x, np.float64)
    m = np.ones(x.shape) if mask is None else (1.0 - mask if mask_invert else np.asarray(mask, np.float64))
    v = x * m
    return np.array([m.sum(), v.sum(), (v * v).sum()]), np.array([0.0, np.abs(v).sum(), (v * v).sum()])


def masked_normalize(x, mask, stats, eps, unbiased=False, mask_invert=False):
    """(x m - mean) / (sqrt(var) + eps) in float64, unrounded (utils.py:62-67); stats = (n, s, q), the global sums when data-parallel."""
    x = np.asarray(x, np.float64)
    m = np.ones(x.shape) if mask is None else (1.0 - mask if mask_invert else np.asarray(mask, np.float64))
    cnt, s, q = (float(v) for v in stats)
    mean = s / cnt
    var = q / cnt - mean * mean
    if unbiased:
        var *= cnt / (cnt - 1.0)
    return (x * m - mean) / (np.sqrt(var) + eps)


# ================================================================================================ inputs of the GPU tests
CAT_NS = (1, 257, 70001)   # one row; one row past a workgroup; 274 workgroups, the last with 113 rows
CAT_HEADS = ((2,), (18,), (3, 4), (2, 3, 1, 5, 2, 4, 3, 2))  # the last: SRL_MAX_HEADS heads, one of a single action
CAT_AVAIL = ("none", "random", "single", "dead")
CAT_CASES = ([(n, dims, av, 2.0) for n in CAT_NS for dims in CAT_HEADS for av in CAT_AVAIL]
             + [(257, (18,), "random", 8.0), (70001, (18,), "spread30", 8.0)])  # logits 8 randn: probabilities underflow
TAIL = 300              # a batch streamed in pieces: rows [TAIL, n) of a call are sampled again with row0 = TAIL
BIG_ROW0 = (1 << 32) + 5
SAMPLE_SEED, SAMPLE_SEED_HIGH = 1234, (0x9E3779B9 << 32) | 77


@functools.lru_cache(maxsize=4)  # the large cases are tens of megabytes each
def cat_case(n, dims, avail_kind, spread):
    """Host arrays of one categorical case.  avail_kind: "none"; "random": 60 % available and the taken action forced available;
    "single": that plus 5 % of the (row, head) pairs with exactly one available action, which is the one taken (and the pair
    (0, 0)); "dead": that plus 5 % of the pairs with none (and the last head of the last row); "spread30": 30 % available.  Every
    seventh row has its maximum twice in every head of two actions or more (the evaluation pick must be the first), both available
    unless the head is one of the special ones; a quarter of the rows are evaluation rows, every fourteenth among them.  With a
    spread above 2 every eleventh row has an available action whose float32 exp(z - max) is 0 without any mask (exp(-120) is below
    float32's smallest denormal): the sampler must never return it, and it is the LAST action, where the sampler falls back when
    rounding carries u to the top of the CDF."""
    dims = tuple(dims)
    H, A = len(dims), sum(dims)
    rng = np.random.default_rng([n, A, H, CAT_AVAIL.index(avail_kind) if avail_kind in CAT_AVAIL else 9, int(spread)])
    logits = (spread * rng.standard_normal((n, A))).astype(np.float32)
    rows, twice = np.arange(0, n, 7), {}
    for k, s, d in _heads(dims):
        if d >= 2:
            j = twice[k] = np.sort(np.stack([rng.permutation(d)[:2] for _ in rows]), 1)
            top = logits[rows, s:s + d].max(1) + np.float32(1.0)
            logits[rows, s + j[:, 0]] = top
            logits[rows, s + j[:, 1]] = top
    action = np.stack([rng.integers(0, d, n) for d in dims], -1).astype(np.int32)
    avail = None
    if avail_kind != "none":
        avail = rng.random((n, A)) < (0.3 if avail_kind == "spread30" else 0.6)
        single = rng.random((n, H)) < 0.05
        dead = rng.random((n, H)) < 0.05
        single[0, 0] = True
        dead[n - 1, H - 1] = True
        if avail_kind not in ("single", "dead"):
            single[:] = False
        if avail_kind != "dead":
            dead[:] = False
        for k, s, d in _heads(dims):
            avail[single[:, k], s:s + d] = False
            avail[np.arange(n), s + action[:, k]] = True
            if k in twice:  # both maxima available, where the head is not one of the special ones
                keep = ~(single[rows, k] | dead[rows, k])
                avail[rows[keep], s + twice[k][keep, 0]] = True
                avail[rows[keep], s + twice[k][keep, 1]] = True
            avail[dead[:, k], s:s + d] = False
        if spread > 2:  # every eleventh row: an AVAILABLE last action more than 120 below every other logit of its head
            deep = np.arange(3, n, 11)
            for k, s, d in _heads(dims):
                logits[deep, s + d - 1] = logits[deep, s:s + d - 1].min(1) - np.float32(120.0)
                avail[deep, s + d - 1] = True
        avail = avail.astype(np.uint8)
    is_eval = (rng.random(n) < 0.25).astype(np.uint8)
    is_eval[::14] = 1  # half of the rows with a tie
    return dict(n=n, dims=dims, logits=logits, action=action, avail=avail, d_logp=rng.standard_normal(n).astype(np.float32),
                d_ent=rng.standard_normal(n).astype(np.float32), is_eval=is_eval)


@functools.lru_cache(maxsize=4)  # the large cases are tens of megabytes each
def cat_reference(n, dims, avail_kind, spread, dtype=torch.float64):
    c = cat_case(n, dims, avail_kind, spread)
    return categorical(c["logits"], c["action"], c["avail"], c["dims"], c["d_logp"], c["d_ent"], dtype)


def categorical_errors(got, ref, scales):
    """got (logp, ent, d_logits; any float dtype) against the float64 reference, in units of the scales (a row of dead heads only
    has scale 0: any difference from its exact 0 counts as infinite).  Also counts the elements of d_logits that must be exactly
    zero and are not."""
    err = {}
    for k in ("logp", "ent"):
        if k in got:
            diff = np.abs(np.asarray(got[k], np.float64) - ref[k])
            err[k] = float(np.where(diff == 0, 0.0, diff / np.maximum(scales[k], 1e-300)).max())
    if "d_logits" in got:
        g = np.asarray(got["d_logits"], np.float64)
        live = scales["d_logits"] > 0
        err["d_logits"] = float((np.abs(g - ref["d_logits"])[live] / scales["d_logits"][live]).max()) if live.any() else 0.0
        err["nonzero_where_exactly_zero"] = int((g[~live] != 0).sum())
    return err


def sample_rows(case, seed, offset, row0=0, start=0, fault=None):
    """The host picks for rows [start, n) of a case numbered from row0."""
    av = None if case["avail"] is None else case["avail"][start:]
    return categorical_sample(case["logits"][start:], av, case["is_eval"][start:], case["dims"], seed, offset, row0, fault)


def sample_mismatches(action, ref):
    """(row, head) pairs where `action` is not the host pick, ambiguous pairs aside (evaluation rows are never ambiguous)."""
    return int(((np.asarray(action) != ref["action"]) & ~ref["ambiguous"]).sum())


def underflowed(case):
    """bool [n, sum(dims)]: actions whose float32 exp(z - max) is 0 -- the unavailable ones of a live head (exp(-1e10 - max)) and
    any whose logit lies more than 104 below the head's maximum.  None in a dead head, where every masked logit IS the maximum."""
    z = _masked(case["logits"], case["avail"]).astype(np.float32)
    out = np.zeros(z.shape, bool)
    for k, s, d in _heads(case["dims"]):
        with np.errstate(under="ignore"):
            out[:, s:s + d] = np.exp(z[:, s:s + d] - z[:, s:s + d].max(1, keepdims=True)) == 0
    return out


def sample_forbidden(action, case, start=0):
    """Picks, in rows [start, n), of an action that is unavailable or whose exp(z - max) is 0 in float32, dead heads aside."""
    gone = underflowed(case)[start:]
    rows = np.arange(gone.shape[0])
    return sum(int(gone[rows, s + np.asarray(action)[:, k]].sum()) for k, s, d in _heads(case["dims"]))


# ---- PPO loss
LOSS_NS = (1, 257, 512 * 256 + 37)  # the grid is capped at 512 workgroups: the largest runs the loop's body twice in 37 threads
LOSS_COMBOS = [(vl, cv, dc) for vl in ("mse", "huber", "smoothl1") for cv in (0, 1) for dc in (0, 1)]
LOSS_COMBOS_FEW = [("huber", 1, 0), ("smoothl1", 1, 1), ("mse", 0, 1)]
LOSS_FORMS = ("own", "share")  # local_n = norm_stats[0] / a rank's share of twice the data
LOSS_CASES = ([(257, vd, c, f) for vd in (1, 3) for c in LOSS_COMBOS for f in LOSS_FORMS]
              + [(n, vd, c, f) for n in (1, LOSS_NS[2]) for vd in (1, 3) for c in LOSS_COMBOS_FEW for f in LOSS_FORMS]
              + [(257, 3, ("smoothl1", 1, 1), "one")])  # all rows masked but one


def loss_hparams(combo):
    vl, cv, dc = combo
    return dict(eps_clip=0.2, c_clip=3.0, value_eps_clip=0.2, value_loss_weight=0.5, entropy_bonus_weight=0.01,
                huber_delta=10.0 if vl == "huber" else 1.0, norm_eps=1e-5, dual_clip=dc, clip_value=cv, value_loss=vl)


@functools.lru_cache(maxsize=4)  # the large cases are tens of megabytes each
def loss_case(n, vd, combo, form):
    """`_draw_loss_case`, drawn again while a case of a few hundred elements has one near a branch: there a single flagged element
    is more than a thousandth of the case, and the exclusion is for the large cases, where such elements cannot be avoided."""
    for attempt in range(20):
        c = _draw_loss_case(n, vd, combo, form, attempt)
        if n > 1000:
            return c
        r = ppo_loss(c["inputs"], c["hp"], c["norm_stats"], c["local_n"], 0)
        if not (r["near_p"] | r["near_v"]).any():
            return c
    raise AssertionError("no draw away from every branch")


def _draw_loss_case(n, vd, combo, form, attempt):
    """Inputs of one loss case (twice the rows are drawn; the case is the first half, a rank's share of the whole in form "share").
    log ratio 0.9 randn: 40 % of the ratios below 0.8, 42 % above 1.2, 11 % above c_clip = 3, half of those with a negative advantage;
    v - ret = 1.2 delta randn: 40 % in the linear region of Huber / SmoothL1; v - old = 0.3 randn against a clip of 0.2; 20 % of the rows
    masked.  The mask byte is stored as the mask; the inverted form is 1 - byte.  norm_stats: the masked sums of the case itself
    ("own"), of all 2 n rows ("share", "one"); below 8 rows, where a sample variance means nothing, the generator's moments times
    that count."""
    hp = loss_hparams(combo)
    delta = hp["huber_delta"]
    rng = np.random.default_rng([n, vd, LOSS_COMBOS.index(combo), LOSS_FORMS.index(form) if form in LOSS_FORMS else 2, attempt])
    N = 2 * n
    old_lp = (-1.0 + 0.4 * rng.standard_normal(N)).astype(np.float32)
    new_lp = (old_lp + 0.9 * rng.standard_normal(N)).astype(np.float32)
    value = (2.0 * rng.standard_normal((N, vd))).astype(np.float32)
    old_value = (value + 0.3 * rng.standard_normal((N, vd))).astype(np.float32)
    ret = (value + 1.2 * delta * rng.standard_normal((N, vd))).astype(np.float32)
    adv = (0.5 + 3.0 * rng.standard_normal((N, vd))).astype(np.float32)
    entropy = (1.0 + 0.3 * rng.standard_normal(N)).astype(np.float32)
    mask = (rng.random(N) < 0.8).astype(np.uint8)
    mask[0] = 1
    if form == "one":
        mask[:n] = 0
        mask[n // 2] = 1
    done, trunc = (rng.random(N) < 0.05).astype(np.uint8), (rng.random(N) < 0.02).astype(np.uint8)
    whole = dict(new_lp=new_lp, old_lp=old_lp, value=value, old_value=old_value, adv=adv, ret=ret, entropy=entropy, mask=mask,
                 done=done, truncated=trunc)
    inputs = {k: np.ascontiguousarray(a[:n]) for k, a in whole.items()}
    local_n = float(inputs["mask"].sum())
    if form == "own":
        stats = masked_stats(inputs["adv"], inputs["mask"].astype(np.float64)[:, None] * np.ones((1, vd)))[0]
        stats[0] = local_n
    else:
        stats = masked_stats(adv, mask.astype(np.float64)[:, None] * np.ones((1, vd)))[0]
        stats[0] = float(mask.sum())
    if n < 8:
        stats = np.array([stats[0], stats[0] * vd * 0.5, stats[0] * vd * 9.25])
    return dict(n=n, vd=vd, hp=hp, inputs=inputs, norm_stats=stats, local_n=local_n)


@functools.lru_cache(maxsize=4)  # the large cases are tens of megabytes each
def loss_reference(n, vd, combo, form, dtype=torch.float64):
    c = loss_case(n, vd, combo, form)
    return ppo_loss(c["inputs"], c["hp"], c["norm_stats"], c["local_n"], 0, dtype)


def loss_errors(got, ref):
    """Gradients (d_new_lp, d_value, d_entropy of any float dtype) against the float64 reference on every element not near a branch,
    in units of the per-element scales; masked elements (scale 0) must be exactly 0 and count as infinite otherwise."""
    keep = dict(d_new_lp=~ref["near_p"].any(1), d_value=~ref["near_v"], d_entropy=np.ones(ref["m"].shape, bool))
    err = {}
    for k, ok in keep.items():
        diff = np.abs(np.asarray(got[k], np.float64).reshape(ref[k].shape) - ref[k])[ok]
        sc = ref["scales"][k][ok]
        err[k] = float(np.where(diff == 0, 0.0, diff / np.maximum(sc, 1e-300)).max()) if diff.size else 0.0
    return err


# which measured per-element bound a sum of per-element terms is held to: the term is formed from the same float32 values
TERM_BOUND = dict(policy="d_new_lp", ratio="d_new_lp", value="d_value", entropy="d_entropy")


def loss_term_errors(terms, ref):
    """The ten sums (by LOSS_TERMS name) against the float64 reference.  Returns exact: the terms that must be equal and are not;
    sums: adv / ret errors in units of their sums of magnitudes; and, for policy / value / entropy / ratio, the distance in units of
    term_mag from the interval the flagged elements leave open.  Every expression that meets at a branch point is continuous there:
    within NEAR (relative) of the point the two sides differ by at most NEAR x the sum of their magnitudes <= 2 NEAR x the element's
    magnitude, so a flagged element's contribution is the reference's +- 2 NEAR x its magnitude, whichever side the float32
    evaluation took.  `clip` counts 0 / 1 terms that are exact away from a branch: it lies between the count over the unflagged
    elements and that plus the number of flagged ones, exactly."""
    m = ref["m"][:, None]
    t = ref["terms"]
    exact = [k for k in ("mask", "done", "trunc") if terms[k] != t[k]]
    fl_p, fl_v = ref["near_p"] * m, ref["near_v"] * m
    unflagged_clip = (m * ~ref["near_p"] * ref["clip_elem"]).sum()
    out = dict(exact=exact, sums={k: abs(terms[k] - t[k]) / max(ref["sign_terms"][k], 1e-300) for k in ("adv", "ret")})
    slack = dict(policy=2 * NEAR * (fl_p * ref["elem_mag"]["policy"]).sum(), value=2 * NEAR * (fl_v * ref["elem_mag"]["value"]).sum(),
                 entropy=0.0, ratio=0.0)
    out["terms"] = {k: max(abs(terms[k] - t[k]) - slack[k], 0.0) / max(ref["term_mag"][k], 1e-300) for k in slack}
    out["clip_range"] = (unflagged_clip, unflagged_clip + fl_p.sum())
    return out
