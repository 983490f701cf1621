"""The small kernels of the update path, each called directly through the C ABI and compared with a plain float64 restatement
on the CPU (numpy / torch, written here): PopArt's statistics, update (with and without the head rescale) and maps, the
importance ratio, the diagonal-Gaussian head, SGD / RMSprop, the gradient fold, NHWC pad / crop / 2x2 max-pool and the ring's
stamp -> slot map.  Whole-step fixtures reach them only at CartPole sizes: below one workgroup, ``value_dim <= 2``, contiguous
operands.  The sizes here are the smallest that take every other path: the grid-stride loops past the grid caps, 64 value
channels, pitched views, row offsets, the wrapper's split of more than ``ACCUMULATE_MAX`` sources.

Measured tolerances (``*_F32_CPU_ERR``): the error of torch's own float32 CPU arithmetic against float64 on the inputs of the test,
recorded next to each constant; the device gets four times that (its ``expf`` / ``logf`` are specified to a couple of ulp, libm
gives one)."""
import numpy as np
import pytest
import torch

from srl_amd import hip

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
S = 2048 * 256 + 3  # one element past a whole grid of the kernels capped at 2048 blocks
EPS = 1e-5          # PopArt's epsilon
HALF_LOG_2PI = 0.5 * np.log(2 * np.pi)


def dev(x, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(x))
    if dtype is not None:
        t = t.to(dtype)
    return t.to(DEV).contiguous()


def rel_close(a, b, rtol=1e-5, scale=None):
    """|a-b| <= rtol * max(|b|, scale), as in tests/test_gpu_kernels.py."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = float(np.abs(b).max()) if scale is None else scale
    return bool((np.abs(a - b) <= rtol * np.maximum(np.abs(b), max(scale, 1e-30))).all())


def ulp32(x):
    """Spacing of float32 at |x| (float64 array in, float64 out)."""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def within_ulp32(got, ref64, ulps=1):
    """A float32 result against a float64 reference: at most ``ulps`` float32 steps from the reference (rounding it is half)."""
    return bool((np.abs(got.astype(np.float64) - ref64) <= ulps * ulp32(ref64)).all())


# ------------------------------------------------------------------------------------------------ PopArt statistics
def _col_stats_ref(x, m):
    """float64 [vd, 3] = per column {sum m, sum x m, sum (x m)^2} and, for the tolerance, the sums of the terms' magnitudes."""
    v = x.astype(np.float64) * m[:, None]
    ref = np.stack([np.broadcast_to(m.sum(), (x.shape[1],)), v.sum(0), (v * v).sum(0)], 1)
    mag = np.stack([np.zeros(x.shape[1]), np.abs(v).sum(0), (v * v).sum(0)], 1)
    return ref, mag


@pytest.mark.parametrize("vd", [1, 3, 64])
@pytest.mark.parametrize("n", [1, 257, 512 * 256 + 37])
def test_masked_stats_cols_and_fold(n, vd):
    """Per-column masked sums (one launch per column, 512 blocks at most: the largest n is 37 rows past a whole grid) and their
    fold.  The count is exact; a sum is float64 accumulation of exact float32 terms in some order: n 2^-52 sum|term|."""
    rng = np.random.default_rng(1000 * vd + n % 997)
    x = (3.0 * rng.standard_normal((n, vd)) + 1.0).astype(np.float32)
    mask = (rng.random(n) < 0.7).astype(np.uint8)
    dx = dev(x)
    for name, dmask, invert, m in (("none", None, False, np.ones(n)), ("mask", dev(mask), False, mask.astype(np.float64)),
                                   ("inverted", dev(mask), True, 1.0 - mask), ("all removed", dev(np.zeros(n, np.uint8)), False, np.zeros(n))):
        stats = torch.full((vd, 3), -7.25e9, dtype=torch.float64, device=DEV)  # garbage: the call zeroes it
        hip.masked_stats_cols(dx, dmask, stats, vd, mask_invert=invert)
        got = stats.cpu().numpy()
        ref, mag = _col_stats_ref(x, m)
        assert np.array_equal(got[:, 0], ref[:, 0]), (name, "count")
        assert (np.abs(got - ref) <= n * 2.0**-52 * mag).all(), (name, np.abs(got - ref).max())
        if name == "all removed":
            assert not got.any()
        out = torch.full((3,), 4.5e7, dtype=torch.float64, device=DEV)
        hip.fold_col_stats(stats, vd, out)
        folded = out.cpu().numpy()
        assert folded[0] == got[0, 0], (name, "the count is taken once")
        for j in (1, 2):  # vd float64 additions of the per-column sums
            assert abs(folded[j] - got[:, j].sum()) <= vd * 2.0**-52 * np.abs(got[:, j]).sum(), (name, j)


# ------------------------------------------------------------------------------------------------ PopArt update / rescale
def _mean_std(rms, vd):
    """RunningMeanStd.mean_std (modules/utils.py:139-141) in float64."""
    deb = max(rms[2 * vd], EPS)
    mean = rms[:vd] / deb
    var = np.maximum(rms[vd:2 * vd] / deb - mean * mean, 1e-2)
    return mean, np.sqrt(var)


def _popart_update_ref(stats, beta, rms, w, b, rescale):
    """popart.py:44-51 / utils.py:125-130 in float64; w [vd, in], b [vd] float32 in, float64 out (unrounded)."""
    vd = b.shape[0]
    old_mean, old_std = _mean_std(rms, vd)
    new = rms.copy()
    new[:vd] = beta * rms[:vd] + stats[:, 1] / stats[:, 0] * (1.0 - beta)
    new[vd:2 * vd] = beta * rms[vd:2 * vd] + stats[:, 2] / stats[:, 0] * (1.0 - beta)
    new[2 * vd] = beta * rms[2 * vd] + 1.0 - beta
    w64, b64 = w.astype(np.float64), b.astype(np.float64)
    if rescale:
        new_mean, new_std = _mean_std(new, vd)
        w64 = w64 * (old_std / new_std)[:, None]
        b64 = (old_std * b64 + old_mean - new_mean) / new_std
    return new, w64, b64


@pytest.mark.parametrize("state", ["fresh", "constant", "burnt-in"])
@pytest.mark.parametrize("in_features", [1, 64, 513])
@pytest.mark.parametrize("vd", [1, 3, 64])
def test_popart_update_and_rescale(vd, in_features, state):
    """One workgroup updates the statistics and (rescale) walks the head's vd x in_features weights in strides of 256: 513 is
    past two strides and no multiple of one.  States: all-zero statistics (debiasing term below eps; std 0.1 before, the
    targets' own afterwards), constant targets (variance clamped at 1e-2 on both sides), a long-running state."""
    rng = np.random.default_rng(100 * vd + in_features)
    beta, n = 0.99999, 200
    targets = (2.0 + 3.0 * rng.standard_normal((n, vd)) * (1.0 + np.arange(vd) / vd)).astype(np.float64)
    rms = np.zeros(2 * vd + 1)
    if state == "constant":
        targets = np.broadcast_to(3.0 + np.arange(vd, dtype=np.float64), (n, vd)).copy()
    elif state == "burnt-in":
        deb = 1.0 - beta**50000
        mean, std = 1.0 + rng.standard_normal(vd), 0.5 + 2.0 * rng.random(vd)
        rms = np.concatenate([mean * deb, (std**2 + mean**2) * deb, [deb]])
    m = (rng.random(n) < 0.8).astype(np.float64)
    stats, _ = _col_stats_ref(targets, m)
    w = (rng.standard_normal((vd, in_features)) / np.sqrt(in_features)).astype(np.float32)
    b = (0.3 * rng.standard_normal(vd)).astype(np.float32)
    x = rng.standard_normal((16, in_features))
    for rescale in (0, 1):
        d_rms, d_w, d_b = dev(rms), dev(w), dev(b)
        hip.popart_update(dev(stats), d_rms, vd, beta, EPS, d_w.data_ptr(), d_b.data_ptr(), in_features, rescale)
        g_rms, g_w, g_b = d_rms.cpu().numpy(), d_w.cpu().numpy(), d_b.cpu().numpy()
        r_rms, r_w, r_b = _popart_update_ref(stats, beta, rms, w, b, rescale)
        assert (np.abs(g_rms - r_rms) <= 4 * np.spacing(np.abs(r_rms))).all(), (rescale, np.abs(g_rms - r_rms).max())
        if not rescale:
            assert np.array_equal(g_w.view(np.uint32), w.view(np.uint32)) and np.array_equal(g_b.view(np.uint32), b.view(np.uint32))
            continue
        # both sides round one double
        assert within_ulp32(g_w, r_w), np.abs(g_w - r_w).max()
        assert within_ulp32(g_b, r_b), np.abs(g_b - r_b).max()
        # PopArt's invariant: the de-normalised output is what it was, up to the rounding of W' and b' to float32
        mu0, sd0 = _mean_std(rms, vd)
        mu1, sd1 = _mean_std(g_rms, vd)
        before = (x @ w.astype(np.float64).T + b) * sd0 + mu0
        w1, b1 = g_w.astype(np.float64), g_b.astype(np.float64)
        after = (x @ w1.T + b1) * sd1 + mu1
        bound = 2.0**-23 * (np.abs(x[:, None, :] * w1[None]).sum(-1) + np.abs(b1)) * sd1 * 2
        assert (np.abs(after - before) <= bound).all(), (np.abs(after - before) / bound).max()
        if state == "fresh":
            assert np.allclose(sd0, 0.1) and (sd1 > 1.0).all()
        if state == "constant":
            assert np.allclose(sd1, 0.1)


@pytest.mark.parametrize("vd", [1, 3])
def test_popart_map_both_directions(vd):
    """normalize (clipped at +-5) and denormalize over S elements (S + 1 for three channels: S is no multiple of 3): the 2048
    blocks wrap around once, and with three channels the wrap falls inside a row (2048 * 256 = 2 mod 3), so the channel of an
    element must come from its index, not from its position in the block.  One float32 rounding of the float64 result."""
    n = -(-S // vd)
    rng = np.random.default_rng(vd)
    deb = 0.37
    mean, std = np.array([1.5, -40.0, 0.01])[:vd], np.array([2.0, 0.25, 30.0])[:vd]
    rms = np.concatenate([mean * deb, (std**2 + mean**2) * deb, [deb]])
    r_mean, r_std = _mean_std(rms, vd)
    x = (mean + std * 2.5 * rng.standard_normal((n, vd))).astype(np.float32)  # ~5 % beyond 5 sigma on either side
    x[:4] = (mean + std * np.array([[5.0], [-5.0], [9.0], [-9.0]])).astype(np.float32)
    d_rms, dx = dev(rms), dev(x)
    out = torch.full((n, vd), float("nan"), device=DEV)
    hip.popart_map(dx, d_rms, vd, out, True, EPS)
    z = (x.astype(np.float64) - r_mean) / r_std
    assert (np.abs(z) > 5).mean() > 0.01
    assert within_ulp32(out.cpu().numpy(), np.clip(z, -5.0, 5.0))
    xn = (3.0 * rng.standard_normal((n, vd))).astype(np.float32)
    out.fill_(float("nan"))
    hip.popart_map(dev(xn), d_rms, vd, out, False, EPS)
    assert within_ulp32(out.cpu().numpy(), xn.astype(np.float64) * r_std + r_mean)


# ------------------------------------------------------------------------------------------------ importance ratio
# max |float32 torch.exp - float64 exp| / exp on the CPU over the differences of test_importance_ratio (measured: 6.096e-8 on
# one CPU, 6.209e-8 on another; the device: 8.28e-8)
EXP_F32_CPU_ERR = 6.21e-8


def _ratio_inputs():
    rng = np.random.default_rng(5)
    old = (-3.0 * rng.random(S)).astype(np.float32)
    new = (old + rng.uniform(-20.0, 20.0, S)).astype(np.float32)
    new[::1000] = old[::1000]  # exact zeros
    new[1], new[2] = old[1] + np.float32(20.0), old[2] - np.float32(20.0)
    d32 = new - old  # the float32 difference the kernel forms
    return new, old, d32


def test_importance_ratio():
    """exp(new - old) over S elements (2048 blocks wrap around once), differences in [-20, 20] with exact zeros, against the
    float64 exponential of the float32 difference."""
    new, old, d32 = _ratio_inputs()
    assert d32.min() < -19.9 and d32.max() > 19.9 and (d32 == 0).sum() >= S // 1000
    ref = np.exp(d32.astype(np.float64))
    cpu = torch.exp(torch.from_numpy(d32)).numpy().astype(np.float64)
    print("float32 CPU exp, max relative error:", (np.abs(cpu - ref) / ref).max())
    out = torch.full((S,), float("nan"), device=DEV)
    hip.importance_ratio(dev(new), dev(old), out)
    got = out.cpu().numpy().astype(np.float64)
    err = np.abs(got - ref) / ref
    print("device, max relative error:", err.max())
    assert err.max() <= 4 * EXP_F32_CPU_ERR, err.max()
    assert (got[d32 == 0] == 1.0).all()


# ------------------------------------------------------------------------------------------------ diagonal Gaussian head
# Errors of float32 torch.distributions.Normal on the CPU against float64, relative to the row's error scale, maximum over the
# shapes and layouts of test_gaussian_fwd_bwd (measured: log-prob 2.422e-7, entropy 1.286e-7, d mean 2.845e-7, d log sigma 3.900e-7
# on one CPU; 2.372e-7, 1.286e-7, 2.918e-7, 4.000e-7 on another -- the larger of each; the device: 2.56e-7, 1.61e-7, 3.38e-7, 3.07e-7)
NORMAL_F32_CPU_ERR = dict(logp=2.43e-7, ent=1.29e-7, d_mean=2.92e-7, d_log_std=4.00e-7)

GAUSS_SHAPES = [(n, A) for n in (1, 257, 70001) for A in (1, 3, 17)]  # 70001 x 17 elements: past the 4096 blocks of the backward
LAYOUTS = ["shared", "per-row", "pitched"]  # log sigma one vector (ld 0) / one row per sample / the same with a pitch of its own


def _gauss_case(n, A, layout, seed):
    """Host arrays of one case: the mean is a column window of a wider matrix (ld_mean > A) in every layout."""
    rng = np.random.default_rng(seed)
    wide = rng.standard_normal((n, A + 5)).astype(np.float32)
    if layout == "shared":
        ls_store = rng.uniform(-5.0, 2.0, (1, A)).astype(np.float32)
        ls, ld_ls, ls_off = np.broadcast_to(ls_store, (n, A)), 0, 0
    elif layout == "per-row":
        ls_store = rng.uniform(-5.0, 2.0, (n, A)).astype(np.float32)
        ls, ld_ls, ls_off = ls_store, A, 0
    else:
        ls_store = rng.uniform(-5.0, 2.0, (n, A + 3)).astype(np.float32)
        ls, ld_ls, ls_off = ls_store[:, 1:1 + A], A + 3, 1
    mean = wide[:, 2:2 + A]
    action = (mean + np.exp(ls) * 1.5 * rng.standard_normal((n, A))).astype(np.float32)
    return dict(n=n, A=A, wide=wide, mean=mean, ls_store=ls_store, ls=np.array(ls), ld_ls=ld_ls, ls_off=ls_off,
                action=action, d_logp=rng.standard_normal(n).astype(np.float32), d_ent=rng.standard_normal(n).astype(np.float32))


def _gauss_device(c):
    d_wide, d_ls = dev(c["wide"]), dev(c["ls_store"])
    return dict(wide=d_wide, ls=d_ls, mean_ptr=d_wide.data_ptr() + 4 * 2, ld_mean=c["A"] + 5, ls_ptr=d_ls.data_ptr() + 4 * c["ls_off"])


def _normal(c, dtype):
    """torch.distributions.Normal and its autograd in ``dtype``: log-prob and entropy [n], d mean and d log sigma [n, A]."""
    mean = torch.from_numpy(np.ascontiguousarray(c["mean"])).to(dtype).requires_grad_(True)
    ls = torch.from_numpy(c["ls"]).to(dtype).requires_grad_(True)
    dist = torch.distributions.Normal(mean, ls.exp())
    logp = dist.log_prob(torch.from_numpy(c["action"]).to(dtype)).sum(-1)
    ent = dist.entropy().sum(-1)
    (logp * torch.from_numpy(c["d_logp"]).to(dtype) + ent * torch.from_numpy(c["d_ent"]).to(dtype)).sum().backward()
    return dict(logp=logp.detach().double().numpy(), ent=ent.detach().double().numpy(), d_mean=mean.grad.double().numpy(),
                d_log_std=ls.grad.double().numpy())


def _gauss_scales(c):
    """What each result is a sum of, in magnitudes: a float32 evaluation is off by a few 2^-24 of these."""
    ls = c["ls"].astype(np.float64)
    d = c["action"].astype(np.float64) - c["mean"].astype(np.float64)
    q = d * d / np.exp(2 * ls)
    dl, de = np.abs(c["d_logp"].astype(np.float64))[:, None], np.abs(c["d_ent"].astype(np.float64))[:, None]
    return dict(logp=(q / 2 + np.abs(ls) + HALF_LOG_2PI).sum(-1), ent=(0.5 + HALF_LOG_2PI + np.abs(ls)).sum(-1),
                d_mean=dl * np.abs(d) / np.exp(2 * ls), d_log_std=dl * (q + 1.0) + de)


def _gauss_errors(got, ref, scales):
    # (a scale is zero only where every term is: an action that rounded onto its mean has a zero gradient on both sides)
    return {k: float((np.abs(got[k].astype(np.float64) - ref[k]) / np.maximum(scales[k], 1e-300)).max()) for k in ref}


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n,A", GAUSS_SHAPES)
def test_gaussian_fwd_bwd(n, A, layout):
    """Log-probability, entropy and their gradients against float64 torch.distributions.Normal and its autograd."""
    c = _gauss_case(n, A, layout, seed=n + A)
    d = _gauss_device(c)
    ref, scales = _normal(c, torch.float64), _gauss_scales(c)
    print("float32 CPU Normal:", _gauss_errors(_normal(c, torch.float32), ref, scales))
    action = dev(c["action"])
    logp, ent = torch.full((n,), float("nan"), device=DEV), torch.full((n,), float("nan"), device=DEV)
    st = hip._stream()
    hip._check(hip.lib().srl_gaussian_fwd(st, d["mean_ptr"], d["ld_mean"], d["ls_ptr"], c["ld_ls"], action.data_ptr(), n, A,
                                          logp.data_ptr(), ent.data_ptr()), "srl_gaussian_fwd")
    d_mean, d_ls = torch.full((n, A), float("nan"), device=DEV), torch.full((n, A), float("nan"), device=DEV)
    d_logp, d_ent = dev(c["d_logp"]), dev(c["d_ent"])
    hip._check(hip.lib().srl_gaussian_bwd(st, d["mean_ptr"], d["ld_mean"], d["ls_ptr"], c["ld_ls"], action.data_ptr(), n, A,
                                          d_logp.data_ptr(), d_ent.data_ptr(), d_mean.data_ptr(), d_ls.data_ptr()),
               "srl_gaussian_bwd")
    got = dict(logp=logp.cpu().numpy(), ent=ent.cpu().numpy(), d_mean=d_mean.cpu().numpy(), d_log_std=d_ls.cpu().numpy())
    err = _gauss_errors(got, ref, scales)
    print("device:", err)
    for k, e in err.items():
        assert e <= 4 * NORMAL_F32_CPU_ERR[k], (k, e)


def _sample(c, d, is_eval, seed, offset, rows=slice(None), row0=0):
    """srl_gaussian_sample on rows ``rows`` of the case (numbered from ``row0`` in the whole batch): (action, logp) on the host."""
    lo = rows.start or 0
    n = (c["n"] if rows.stop is None else rows.stop) - lo
    A = c["A"]
    action, logp = torch.full((n, A), float("nan"), device=DEV), torch.full((n,), float("nan"), device=DEV)
    ev = dev(is_eval[rows])
    hip._check(hip.lib().srl_gaussian_sample(hip._stream(), d["mean_ptr"] + 4 * lo * d["ld_mean"], d["ld_mean"],
                                             d["ls_ptr"] + 4 * lo * c["ld_ls"], c["ld_ls"], ev.data_ptr(), n, A, seed, offset,
                                             action.data_ptr(), logp.data_ptr(), row0), "srl_gaussian_sample")
    return action.cpu().numpy(), logp.cpu().numpy()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n,A", GAUSS_SHAPES)
def test_gaussian_sample(n, A, layout):
    c = _gauss_case(n, A, layout, seed=7 * n + A)
    d = _gauss_device(c)
    rng = np.random.default_rng(n)
    is_eval = (rng.random(n) < 0.25).astype(np.uint8)
    action, logp = _sample(c, d, is_eval, seed=1234, offset=5)
    assert np.isfinite(action).all() and np.isfinite(logp).all()
    ev = is_eval.astype(bool)
    assert np.array_equal(action[ev].view(np.uint32), np.ascontiguousarray(c["mean"][ev]).view(np.uint32)), "evaluation: the mean"
    # the returned log-probability is the float64 log-density of the returned action, at the forward kernel's tolerance
    ref = _normal(dict(c, action=action), torch.float64)["logp"]
    scale = _gauss_scales(dict(c, action=action))["logp"]
    assert (np.abs(logp - ref) / scale).max() <= 4 * NORMAL_F32_CPU_ERR["logp"], (np.abs(logp - ref) / scale).max()
    # another offset (the next rollout call), other draws
    other, _ = _sample(c, d, is_eval, seed=1234, offset=6)
    assert np.array_equal(other[ev], action[ev])
    if (~ev).any():
        assert (other[~ev] != action[~ev]).mean() > 0.99
    k = 300  # a batch streamed in pieces: rows [k, n) numbered from k draw what they draw in the whole batch
    if n > k:
        tail_a, tail_l = _sample(c, d, is_eval, seed=1234, offset=5, rows=slice(k, None), row0=k)
        assert np.array_equal(tail_a.view(np.uint32), action[k:].view(np.uint32))
        assert np.array_equal(tail_l.view(np.uint32), logp[k:].view(np.uint32))
        shifted, _ = _sample(c, d, is_eval, seed=1234, offset=5, rows=slice(k, None), row0=0)
        assert (shifted[~ev[k:]] != action[k:][~ev[k:]]).mean() > 0.99, "row0 is part of the counter"


def test_gaussian_sample_moments():
    """Standardised draws at n = 70001, A = 3 (N = 210003 numbers from a fixed seed, so the run is deterministic): mean, variance
    and the pairwise column correlations within five standard deviations of their estimators (1/sqrt(N), sqrt(2/N), 1/sqrt(n)).
    Checked on the CPU first: numpy's own normal generator at the same N, seeds 0..199, reaches |mean| sqrt(N) = 2.68,
    |var - 1| sqrt(N/2) = 3.31 and |corr| sqrt(n) = 3.69 at most -- a correct sampler stays inside five, one whose columns or
    rows share counters does not."""
    n, A = 70001, 3
    c = _gauss_case(n, A, "per-row", seed=99)
    d = _gauss_device(c)
    action, _ = _sample(c, d, np.zeros(n, np.uint8), seed=20240229, offset=11)
    z = (action.astype(np.float64) - c["mean"]) / np.exp(c["ls"].astype(np.float64))
    N = n * A
    assert abs(z.mean()) <= 5 / np.sqrt(N), z.mean()
    assert abs(z.var() - 1.0) <= 5 * np.sqrt(2.0 / N), z.var()
    corr = np.corrcoef(z.T)
    for i in range(A):
        for j in range(i + 1, A):
            assert abs(corr[i, j]) <= 5 / np.sqrt(n), (i, j, corr[i, j])
    # neighbouring rows do not share draws either
    assert abs(np.corrcoef(z[:-1, 0], z[1:, 0])[0, 1]) <= 5 / np.sqrt(n)


# ------------------------------------------------------------------------------------------------ SGD / RMSprop
def _optim_run(n, make_opt, step_fn, state_names, centered=False):
    """Three steps of a torch optimiser on the CPU against the kernel, in the three modes every variant runs in: no clipping,
    clipping, and clipping of gradients scaled by 0.5 (the data-parallel mean).  test_adam_matches_torch's pattern and bounds."""
    for mode, max_norm, gscale in (("plain", None, 1.0), ("clip", 0.005 * np.sqrt(n), 1.0), ("scaled", 0.002 * np.sqrt(n), 0.5)):
        rng = np.random.default_rng(n % 1000 + 17)
        p0 = rng.standard_normal(n).astype(np.float32)
        tp = torch.from_numpy(p0.copy()).requires_grad_(True)
        opt = make_opt([tp])
        p = dev(p0).clone()
        state = {k: torch.full((n,), float("nan"), device=DEV) if k == "nan" else torch.zeros(n, device=DEV) for k in state_names}
        sumsq = torch.zeros(1, dtype=torch.float64, device=DEV)
        gn = torch.zeros(1, device=DEV)
        for step in range(1, 4):
            g = rng.standard_normal(n).astype(np.float32) * 0.01
            tp.grad = torch.from_numpy(g * np.float32(gscale))
            ref_norm = torch.nn.utils.clip_grad_norm_([tp], max_norm if max_norm is not None else 1e30)
            opt.step()
            dg = dev(g)
            hip.grad_sumsq(dg, sumsq)
            step_fn(p, dg, state, step, dict(grad_scale=gscale, max_norm=-1 if max_norm is None else max_norm, sumsq=sumsq,
                                             grad_norm_out=gn))
            assert abs(gn.item() - ref_norm.item()) <= 1e-5 * ref_norm.item(), (mode, step)
            assert rel_close(p.cpu().numpy(), tp.detach().numpy(), 1e-6, scale=1.0), (mode, step, np.abs(p.cpu().numpy() - tp.detach().numpy()).max())
            if centered:  # the square root under test is well conditioned, so the comparison says something
                st = opt.state[tp]
                sq, ga = st["square_avg"].double(), st["grad_avg"].double()
                assert bool((sq - ga * ga >= 1e-3 * sq).all()), (mode, step)


SGD_VARIANTS = {
    "plain": dict(lr=1e-2),
    "momentum": dict(lr=1e-2, momentum=0.9),
    "dampening": dict(lr=1e-2, momentum=0.8, dampening=0.3),
    "nesterov-wd": dict(lr=1e-2, momentum=0.9, nesterov=True, weight_decay=1e-3),
    # the first step sets the buffer to the gradient -- undamped, whatever the buffer held (here: NaN) -- later ones blend
    "first-step": dict(lr=1e-2, momentum=0.8, dampening=0.3),
}


@pytest.mark.parametrize("n", [1, 100003, S])
@pytest.mark.parametrize("variant", list(SGD_VARIANTS))
def test_sgd_matches_torch(variant, n):
    cfg = SGD_VARIANTS[variant]
    mom, damp = cfg.get("momentum", 0.0), cfg.get("dampening", 0.0)

    def step_fn(p, g, state, step, clip):
        hip.sgd_step(p, g, state.get("buf", state.get("nan")), cfg["lr"], mom, damp, cfg.get("weight_decay", 0.0),
                     cfg.get("nesterov", False), step == 1, **clip)

    names = [] if mom == 0 else (["nan"] if variant == "first-step" else ["buf"])
    _optim_run(n, lambda ps: torch.optim.SGD(ps, **cfg), step_fn, names)


RMS_VARIANTS = {
    "plain": dict(lr=1e-2),
    "momentum": dict(lr=1e-3, momentum=0.9),
    "centered": dict(lr=1e-2, alpha=0.95, centered=True),
    # eps 1e-3: with weight decay the gradient g + wd p is itself a rounded sum, and g / (c |g| + eps) has slope 1 / eps where
    # that sum cancels.  On these inputs torch's own float32 step is 2.3e-6 (eps 1e-6) or 2e-4 (eps 1e-8) away from its float64
    # step at n = S, 1.7e-7 with eps 1e-3: only there does a bound of 1e-6 compare implementations and not rounding orders
    "centered-momentum-wd": dict(lr=5e-4, alpha=0.95, eps=1e-3, momentum=0.9, centered=True, weight_decay=1e-3),
}


@pytest.mark.parametrize("n", [1, 100003, S])
@pytest.mark.parametrize("variant", list(RMS_VARIANTS))
def test_rmsprop_matches_torch(variant, n):
    cfg = RMS_VARIANTS[variant]
    mom, cen = cfg.get("momentum", 0.0), cfg.get("centered", False)

    def step_fn(p, g, state, step, clip):
        hip.rmsprop_step(p, g, state["sq"], state.get("buf"), state.get("gavg"), cfg["lr"], cfg.get("alpha", 0.99),
                         cfg.get("eps", 1e-8), cfg.get("weight_decay", 0.0), mom, cen, **clip)

    names = ["sq"] + (["buf"] if mom > 0 else []) + (["gavg"] if cen else [])
    _optim_run(n, lambda ps: torch.optim.RMSprop(ps, **cfg), step_fn, names, centered=cen)


# ------------------------------------------------------------------------------------------------ gradient fold
@pytest.mark.parametrize("k", [1, 2, hip.ACCUMULATE_MAX, hip.ACCUMULATE_MAX + 3])
def test_accumulate_n_adds_left_to_right(k):
    """dst += src_0 + ... + src_{k-1} over S elements, bit-equal to adding the sources one by one in float32 (what the header
    promises); more than ACCUMULATE_MAX sources go through in two launches and must still be that sum."""
    rng = np.random.default_rng(k)
    dst = rng.standard_normal(S).astype(np.float32)
    srcs = [(rng.standard_normal(S) * 10.0**rng.integers(-3, 4)).astype(np.float32) for _ in range(k)]
    ref = dst.copy()
    for s in srcs:
        ref = ref + s
    d = dev(dst)
    hip.accumulate_n(d, [dev(s) for s in srcs])
    assert np.array_equal(d.cpu().numpy().view(np.uint32), ref.view(np.uint32))


# ------------------------------------------------------------------------------------------------ NHWC pad / crop / max-pool
# (an image is the D = 1 case of the channels-last volume kernels)
@pytest.mark.parametrize("pad", [1, 2])
@pytest.mark.parametrize("H,W,C", [(7, 5, 1), (9, 11, 3), (5, 7, 32)])
def test_pad_crop_nhwc(H, W, C, pad):
    rng = np.random.default_rng(H * W + C + pad)
    n = 3
    x = rng.standard_normal((n, H, W, C)).astype(np.float32)
    ref = torch.nn.functional.pad(torch.from_numpy(x).permute(0, 3, 1, 2), (pad,) * 4).permute(0, 2, 3, 1).numpy()
    dx = dev(x)
    y = torch.full((n, H + 2 * pad, W + 2 * pad, C), float("nan"), device=DEV)
    hip.pad_ndhwc(dx.data_ptr(), n, (1, H, W, C), (0, pad, pad), y.data_ptr())
    assert np.array_equal(y.cpu().numpy(), ref)
    back = torch.full((n, H, W, C), float("nan"), device=DEV)
    hip.crop_ndhwc(y.data_ptr(), n, (1, H, W, C), (0, pad, pad), back.data_ptr())
    assert np.array_equal(back.cpu().numpy(), x), "crop(pad(x)) == x"
    # crop is the adjoint of the zero padding: the interior of any padded gradient
    dy = rng.standard_normal((n, H + 2 * pad, W + 2 * pad, C)).astype(np.float32)
    ddy = dev(dy)
    hip.crop_ndhwc(ddy.data_ptr(), n, (1, H, W, C), (0, pad, pad), back.data_ptr())
    assert np.array_equal(back.cpu().numpy(), dy[:, pad:-pad, pad:-pad])


@pytest.mark.parametrize("dact", [0, 1, 2])
@pytest.mark.parametrize("H,W,C", [(7, 5, 1), (9, 11, 3), (5, 7, 32)])
def test_maxpool2_nhwc_matches_torch(H, W, C, dact):
    """MaxPool2d(2) on odd extents (the trailing row and column are dropped and get no gradient) and its backward: the gradient
    goes to the FIRST maximum of a window in scan order (torch's rule), times the derivative of the activation that made x.
    Ties are frequent (quantised input) and one plane is constant, so every window of it is a four-way tie."""
    rng = np.random.default_rng(H * W + C + dact)
    n = 4
    x = np.round(rng.standard_normal((n, H, W, C)) * 2).astype(np.float32) / 2
    x[0, :, :, 0] = 0.5
    if dact == 1:
        x = np.maximum(x, 0)
    elif dact == 2:
        x = np.tanh(x).astype(np.float32)
    xt = torch.from_numpy(x).permute(0, 3, 1, 2).clone().requires_grad_(True)
    yt = torch.nn.functional.max_pool2d(xt, 2)
    OH, OW = H // 2, W // 2
    dx = dev(x)
    y = torch.full((n, OH, OW, C), float("nan"), device=DEV)
    hip.maxpool_ndhwc_fwd(dx.data_ptr(), n, (1, H, W, C), (1, 2, 2), y.data_ptr())
    assert np.array_equal(y.cpu().numpy(), yt.detach().permute(0, 2, 3, 1).numpy())
    dy = rng.standard_normal((n, OH, OW, C)).astype(np.float32)
    dy[dy == 0] = 1.0
    (yt * torch.from_numpy(dy).permute(0, 3, 1, 2)).sum().backward()
    routed = xt.grad.permute(0, 2, 3, 1).numpy()  # float32: one dy per window, nothing is summed
    assert (routed[0, :2 * OH:2, :2 * OW:2, 0] == dy[0, :, :, 0]).all(), "torch routes a tie to the first element"
    out = torch.full((n, H, W, C), float("nan"), device=DEV)
    ddy = dev(dy)
    hip.maxpool_ndhwc_bwd(ddy.data_ptr(), dx.data_ptr(), n, (1, H, W, C), (1, 2, 2), dact, out.data_ptr())
    got = out.cpu().numpy()
    if dact == 0:
        assert np.array_equal(got, routed)
    elif dact == 1:
        assert np.array_equal(got, routed * (x > 0))
    else:  # which element receives the gradient: exactly; its value: 1 - x^2 may be one fused operation on the device
        assert np.array_equal(got != 0, (routed != 0) & (np.abs(x) < 1))
        assert rel_close(got, routed.astype(np.float64) * (1.0 - x.astype(np.float64)**2), 1e-6, scale=1.0)


# ------------------------------------------------------------------------------------------------ ring stamps -> slots
@pytest.mark.parametrize("capacity", [1, 7, 4096])
def test_ring_slots_is_pythons_modulo(capacity):
    """(stamp - base) % capacity with Python's sign convention, for stamps below, at and above the base over several
    capacities' worth of sequence numbers, and with the ring's generation in the high bits of the base."""
    rng = np.random.default_rng(capacity)
    for base in (0, 1, (3 << 40) + 1):
        lo = max(base - 3 * capacity - 2, -(1 << 62))
        stamps = np.concatenate([np.arange(lo, base + 3 * capacity + 3), [base], rng.integers(lo, base + 50 * capacity, 4096 * 256 + 5)])
        stamps = stamps.astype(np.int64)
        out = torch.full((stamps.size,), -1, dtype=torch.int32, device=DEV)
        hip.ring_slots(dev(stamps), capacity, out, base=base)
        ref = np.array([(int(s) - base) % capacity for s in stamps[:6 * capacity + 6]], dtype=np.int64)
        got = out.cpu().numpy().astype(np.int64)
        assert np.array_equal(got[:ref.size], ref), (base, "below / at / above the base")
        assert np.array_equal(got, np.mod(stamps - base, capacity)), base
