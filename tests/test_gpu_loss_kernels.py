"""The discrete-action heads, their Philox sampler, the PPO loss and the masked normalisation -- the kernels every update of every
discrete-action configuration passes through (csrc/categorical.hip, csrc/ppo_loss.hip, csrc/gae.hip; the head arithmetic, the
Philox draw and the value loss they share: csrc/action_dist.h) -- each called through the raw C entry points, so
that pitches can differ from widths, and compared with the float64 restatements of tests/loss_ref.py at the sizes where such
kernels go wrong: one row, one row past a workgroup, past the grid caps (512 workgroups of the loss, 2048 of the normalisation),
SRL_MAX_HEADS heads, a head of one action, heads with one or no available action, column windows of wider matrices.  Outputs are
pre-filled with NaN (or a sentinel) and everything outside a window must stay as it was.

Tolerances (``*_F32_CPU_ERR``): the largest error of the float32 CPU run of the same restatement against its float64 run on the
inputs of the tests, in units of the per-element error scale (loss_ref.py), recorded next to each constant; the device gets four
times that (its ``expf`` / ``logf`` are specified to a couple of ulp, libm gives one).  tests/test_loss_reference.py shows on these
inputs that the bounds can fail and that the exclusions (sampling: ambiguous picks; loss: elements near a branch) stay below a
thousandth."""
import numpy as np
import pytest
import torch

import loss_ref as R
from srl_amd import hip
from test_gpu_small_kernels import within_ulp32

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")

# Errors of the float32 CPU run of loss_ref.categorical against its float64 run, in units of the error scales, maximum over
# loss_ref.CAT_CASES (measured: log-prob 1.178e-7, entropy 1.352e-7, d logits 1.806e-7, the same on two CPUs; the device, over the
# three layouts: 1.43e-7, 8.60e-8, 1.43e-7; the log-prob the sampler returns: 1.47e-7)
CAT_F32_CPU_ERR = dict(logp=1.18e-7, ent=1.36e-7, d_logits=1.81e-7)
# The same of loss_ref.ppo_loss over loss_ref.LOSS_CASES, on the elements not near a branch (measured: d new_lp 2.758e-7, d value
# 1.517e-7, d entropy 8.076e-8, the same on two CPUs; the device: 2.81e-7, 1.52e-7, 8.08e-8 -- the value and entropy gradients hold no
# transcendental, so IEEE arithmetic gives the device what it gives the CPU).  The sums, in units of their sums of magnitudes:
# float32 CPU policy 8.82e-8, value 3.29e-8, ratio 4.44e-8, entropy 0; the device the same; adv / ret on the device: 3.8e-17
LOSS_F32_CPU_ERR = dict(d_new_lp=2.76e-7, d_value=1.52e-7, d_entropy=8.08e-8)
SUM_TOL = 1e-12  # a float64 sum of exact float32 terms in another order: n 2^-53 of the sum of magnitudes at the very most


def dev(x, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(x))
    if dtype is not None:
        t = t.to(dtype)
    return t.to(DEV).contiguous()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _case_id(c):
    return "-".join("x".join(map(str, v)) if isinstance(v, tuple) else str(v) for v in c)


# ------------------------------------------------------------------------------------------------ categorical heads
CAT_LAYOUTS = ("contiguous", "window", "window+pitched-grad")
LOGIT_PAD, LOGIT_OFF, GRAD_PAD, GRAD_OFF = 5, 2, 3, 1  # the window starts at column 2 of A + 5; the gradient's at 1 of A + 3


def _logits_on_device(c, layout):
    """(tensor kept alive, pointer to the first logit, pitch): contiguous, or a column window of a wider matrix of NaN -- a kernel
    that reads beside the window returns NaN."""
    A = c["logits"].shape[1]
    if layout == "contiguous":
        t = dev(c["logits"])
        return t, t.data_ptr(), A
    wide = np.full((c["n"], A + LOGIT_PAD), np.nan, np.float32)
    wide[:, LOGIT_OFF:LOGIT_OFF + A] = c["logits"]
    t = dev(wide)
    return t, t.data_ptr() + 4 * LOGIT_OFF, A + LOGIT_PAD


def _cat_device(c, layout):
    n, dims = c["n"], c["dims"]
    A, H = sum(dims), len(dims)
    keep, lg_ptr, ld = _logits_on_device(c, layout)
    action, avail = dev(c["action"]), None if c["avail"] is None else dev(c["avail"])
    logp, ent = torch.full((n,), NAN, device=DEV), torch.full((n,), NAN, device=DEV)
    st, hd = hip._stream(), hip._i32_array(dims)
    hip._check(hip.lib().srl_categorical_fwd(st, lg_ptr, ld, action.data_ptr(), _ptr(avail), n, H, hd, logp.data_ptr(), ent.data_ptr()),
               "srl_categorical_fwd")
    pad, off = (GRAD_PAD, GRAD_OFF) if layout == "window+pitched-grad" else (0, 0)
    d_wide = torch.full((n, A + pad), NAN, device=DEV)
    d_logp, d_ent = dev(c["d_logp"]), dev(c["d_ent"])
    hip._check(hip.lib().srl_categorical_bwd(st, lg_ptr, ld, action.data_ptr(), _ptr(avail), n, H, hd, d_logp.data_ptr(), d_ent.data_ptr(),
                                             d_wide.data_ptr() + 4 * off, A + pad), "srl_categorical_bwd")
    d_all = d_wide.cpu().numpy()
    outside = np.ones(A + pad, bool)
    outside[off:off + A] = False
    assert np.isnan(d_all[:, outside]).all(), "columns outside the gradient's window are the caller's"
    return dict(logp=logp.cpu().numpy(), ent=ent.cpu().numpy(), d_logits=d_all[:, off:off + A])


@pytest.mark.parametrize("case", R.CAT_CASES, ids=_case_id)
def test_categorical_fwd_bwd_float64(case):
    """Log-probability, entropy and d logits against float64 torch.distributions.Categorical and its autograd, in the three
    layouts.  Exactly zero gradient at unavailable actions and in dead heads; with one available action log-prob and entropy are 0
    and the gradient vanishes within the tolerance (the reference's values there, nothing special-cased); a dead head adds
    exactly 0 to both, as float32 arithmetic next to -1e10 makes it (derived in loss_ref.categorical; exact arithmetic would add
    -log d and log d), so the live heads of its row are held to their own scale."""
    c = R.cat_case(*case)
    ref, sc = R.cat_reference(*case)
    print("\nfloat32 CPU Categorical:", R.categorical_errors(R.cat_reference(*case, torch.float32)[0], ref, sc))
    for layout in CAT_LAYOUTS:
        got = _cat_device(c, layout)
        assert np.isfinite(got["logp"]).all() and np.isfinite(got["ent"]).all() and np.isfinite(got["d_logits"]).all(), layout
        err = R.categorical_errors(got, ref, sc)
        print(f"device, {layout}:", err)
        assert err["nonzero_where_exactly_zero"] == 0, layout
        for k, bound in CAT_F32_CPU_ERR.items():
            assert err[k] <= 4 * bound, (layout, k, err[k])


def _sample_device(c, layout, seed, offset, row0=0, start=0):
    """srl_categorical_sample on rows [start, n) of the case, numbered from row0: (action int64 [rows, heads], logp [rows])."""
    n, dims = c["n"] - start, c["dims"]
    H = len(dims)
    keep, lg_ptr, ld = _logits_on_device(c, layout)
    avail = None if c["avail"] is None else dev(c["avail"][start:])
    is_eval = dev(c["is_eval"][start:])
    action = torch.full((n, H), -7, dtype=torch.int64, device=DEV)
    logp = torch.full((n,), NAN, device=DEV)
    hip._check(hip.lib().srl_categorical_sample(hip._stream(), lg_ptr + 4 * start * ld, ld, _ptr(avail), is_eval.data_ptr(), n, H,
                                                hip._i32_array(dims), seed, offset, action.data_ptr(), logp.data_ptr(), row0),
               "srl_categorical_sample")
    return action.cpu().numpy(), logp.cpu().numpy()


@pytest.mark.parametrize("case", R.CAT_CASES, ids=_case_id)
def test_categorical_sample_follows_the_host_sampler(case):
    """The device's picks are the host's float64 inverse-CDF picks from the same Philox counters on every (row, head) that is not
    within rounding of a CDF boundary (evaluation rows never are: the first maximum, exactly); never an unavailable action; the
    returned log-probability is that of the returned action.  The counter layout is pinned word by word: the head (multi-head
    cases), the offset (5 and 6 against their own host picks; 5 + 2^32 is 5: only the low word enters), the row's number in the
    whole batch (a tail sampled with row0 = TAIL is bitwise the tail of the whole call; row0 past 2^32 reaches the high word) and
    both words of the seed.

    Two draws from one distribution coincide with probability sum p^2 (about a fifth for the 18-way head of these cases), so
    the ACTIONS at offsets 5 and 6 cannot differ on 99 % of the rows; the draws do: tests/test_loss_reference.py asserts that the
    host's uniforms differ on > 99 % of the sampled rows, and here the device follows the host at both offsets and its own picks
    at the two offsets differ."""
    c = R.cat_case(*case)
    n, dims = c["n"], c["dims"]
    seed = R.SAMPLE_SEED
    host = R.sample_rows(c, seed, 5)
    for layout in CAT_LAYOUTS[:2]:
        act, lp = _sample_device(c, layout, seed, 5)
        assert ((act >= 0) & (act < np.array(dims))).all(), layout
        assert R.sample_mismatches(act, host) == 0, (layout, R.sample_mismatches(act, host))
        assert R.sample_forbidden(act, c) == 0, layout
        ref, sc = R.categorical(c["logits"], act, c["avail"], dims)
        err = R.categorical_errors(dict(logp=lp), ref, sc)["logp"]
        print(f"\ndevice, {layout}: log-prob of the returned action", err, "ambiguous", int(host["ambiguous"].sum()))
        assert err <= 4 * CAT_F32_CPU_ERR["logp"], (layout, err)
    for name, kw in (("offset 6", dict(offset=6)), ("row0 past 2^32", dict(offset=5, row0=R.BIG_ROW0)),
                     ("seed with a high word", dict(offset=5, seed=R.SAMPLE_SEED_HIGH))):
        kw = dict(dict(seed=seed, row0=0), **kw)
        other, _ = _sample_device(c, "window", **kw)
        host_o = R.sample_rows(c, kw["seed"], kw["offset"], kw["row0"])
        assert R.sample_mismatches(other, host_o) == 0, name
        assert R.sample_forbidden(other, c) == 0, name
        ev = c["is_eval"] != 0
        assert np.array_equal(other[ev], act[ev]), (name, "an evaluation row's pick depends on no draw")
        if n >= 257 and 18 in dims:  # on the device itself: another stream, other picks (how many, the host comparison above says)
            assert (other[~ev] != act[~ev]).any(), name
    wrapped, wlp = _sample_device(c, "window", seed, 5 + (1 << 32))
    assert np.array_equal(wrapped, act) and np.array_equal(wlp.view(np.uint32), lp.view(np.uint32)), "only the offset's low word enters"
    if n > R.TAIL:
        tail_a, tail_l = _sample_device(c, "window", seed, 5, row0=R.TAIL, start=R.TAIL)
        assert np.array_equal(tail_a, act[R.TAIL:]), "a batch streamed in pieces samples what it would in one call"
        assert np.array_equal(tail_l.view(np.uint32), lp[R.TAIL:].view(np.uint32))


SHARED_WALK_CASES = [(257, (2, 3, 1, 5, 2, 4, 3, 2), "dead", 2.0),  # a row past a workgroup, SRL_MAX_HEADS heads, dead and single-action heads
                     (257, (18,), "random", 8.0)]                   # probabilities underflow


@pytest.mark.parametrize("case", SHARED_WALK_CASES, ids=_case_id)
def test_entry_points_share_one_head_walk(case):
    """The categorical entry points normalise a head by one definition (csrc/action_dist.h), seen from outside, in the "window"
    layout, bitwise on the float32 patterns: (a) the rows of srl_categorical_log_softmax, gathered at the case's actions and added
    over the heads in float32 in head order from 0, are srl_categorical_fwd's log-probability; (b) the log-probability
    srl_categorical_sample returns is srl_categorical_fwd's log-probability of the actions it returned."""
    c = R.cat_case(*case)
    n, dims = c["n"], c["dims"]
    A, H = sum(dims), len(dims)
    keep, lg_ptr, ld = _logits_on_device(c, "window")
    avail = dev(c["avail"])
    st, hd, L = hip._stream(), hip._i32_array(dims), hip.lib()

    def fwd_logp(action):
        act = dev(action, torch.int32)
        logp, ent = torch.full((n,), NAN, device=DEV), torch.full((n,), NAN, device=DEV)
        hip._check(L.srl_categorical_fwd(st, lg_ptr, ld, act.data_ptr(), avail.data_ptr(), n, H, hd, logp.data_ptr(), ent.data_ptr()),
                   "srl_categorical_fwd")
        return logp.cpu().numpy()

    wide = torch.full((n, A + GRAD_PAD), NAN, device=DEV)
    hip._check(L.srl_categorical_log_softmax(st, lg_ptr, ld, avail.data_ptr(), n, H, hd, wide.data_ptr() + 4 * GRAD_OFF, A + GRAD_PAD),
               "srl_categorical_log_softmax")
    rows = wide.cpu().numpy()[:, GRAD_OFF:GRAD_OFF + A]
    assert rows.dtype == np.float32 and np.isfinite(rows).all()
    gathered = np.zeros(n, np.float32)
    for k, s, d in R._heads(dims):
        gathered = gathered + rows[np.arange(n), s + c["action"][:, k]]  # float32 + float32, rounded once like the kernel's
    assert gathered.dtype == np.float32
    logp = fwd_logp(c["action"])
    diff = np.abs(gathered.astype(np.float64) - logp)
    print(f"\n(a) log-softmax rows gathered against fwd: max difference {diff.max():.3e}")
    assert np.array_equal(gathered.view(np.uint32), logp.view(np.uint32)), ("a", float(diff.max()))
    act, lp = _sample_device(c, "window", R.SAMPLE_SEED, 5)
    again = fwd_logp(act)
    diff = np.abs(lp.astype(np.float64) - again)
    print(f"(b) the sampler's log-probability against fwd at its picks: max difference {diff.max():.3e}")
    assert np.array_equal(lp.view(np.uint32), again.view(np.uint32)), ("b", float(diff.max()))


def test_categorical_argument_errors():
    """What SRL_CHECK_ARG refuses on the host, before any launch: more than SRL_MAX_HEADS heads, a head of no action, a pitch below
    the row's width."""
    c = R.cat_case(257, (3, 4), "random", 2.0)
    n = c["n"]
    lg, action, avail = dev(c["logits"]), dev(c["action"]), dev(c["avail"])
    out, out2 = torch.full((n,), NAN, device=DEV), torch.full((n,), NAN, device=DEV)
    grad = torch.full((n, 7), NAN, device=DEV)
    acts = torch.full((n, 2), -7, dtype=torch.int64, device=DEV)
    st, L = hip._stream(), hip.lib()

    def fwd(H, dims, ld):
        hip._check(L.srl_categorical_fwd(st, lg.data_ptr(), ld, action.data_ptr(), avail.data_ptr(), n, H, hip._i32_array(dims),
                                         out.data_ptr(), out2.data_ptr()), "srl_categorical_fwd")

    def bwd(H, dims, ld, ldd):
        hip._check(L.srl_categorical_bwd(st, lg.data_ptr(), ld, action.data_ptr(), avail.data_ptr(), n, H, hip._i32_array(dims),
                                         out.data_ptr(), out2.data_ptr(), grad.data_ptr(), ldd), "srl_categorical_bwd")

    def sample(H, dims, ld):
        hip._check(L.srl_categorical_sample(st, lg.data_ptr(), ld, avail.data_ptr(), None, n, H, hip._i32_array(dims), 1, 0,
                                            acts.data_ptr(), out.data_ptr(), 0), "srl_categorical_sample")

    nine = [1] * (hip.MAX_HEADS + 1)
    for call in (lambda: fwd(9, nine, 9), lambda: fwd(2, (3, 4), 6), lambda: fwd(2, (3, 0), 7), lambda: bwd(9, nine, 9, 9),
                 lambda: bwd(2, (3, 4), 6, 7), lambda: bwd(2, (3, 4), 7, 6), lambda: sample(9, nine, 9), lambda: sample(2, (3, 4), 6)):
        with pytest.raises(hip.HipError):
            call()
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(grad).all() and bool((acts == -7).all()), "a refused call writes nothing"


# ------------------------------------------------------------------------------------------------ PPO loss
def _hparams(hp, mask_invert):
    kw = dict(hp, value_loss=hip.VALUE_LOSS_KINDS[hp["value_loss"]], mask_invert=int(mask_invert))
    return hip.PpoHparams(**kw)


def _loss_device(c, mask_invert, with_done):
    """srl_ppo_loss_fwd_bwd on the case: the mask byte inverted when mask_invert (the same logical mask), done / truncated NULL
    unless with_done.  Returns the three gradients (numpy) and the ten sums by name."""
    n, vd, inp = c["n"], c["vd"], c["inputs"]
    d = {k: dev(inp[k]) for k in ("new_lp", "old_lp", "value", "old_value", "adv", "ret", "entropy")}
    mask = dev(1 - inp["mask"] if mask_invert else inp["mask"], torch.uint8)
    done, trunc = (dev(inp["done"]), dev(inp["truncated"])) if with_done else (None, None)
    stats, local_n = dev(c["norm_stats"], torch.float64), dev(np.array([c["local_n"]]), torch.float64)
    d_new_lp, d_value, d_ent = torch.full((n,), NAN, device=DEV), torch.full((n, vd), NAN, device=DEV), torch.full((n,), NAN, device=DEV)
    terms = torch.full((hip.LT_COUNT,), 123.0, dtype=torch.float64, device=DEV)  # zeroed by the call, not accumulated into
    hp = _hparams(c["hp"], mask_invert)
    hip._check(hip.lib().srl_ppo_loss_fwd_bwd(hip._stream(), d["new_lp"].data_ptr(), d["old_lp"].data_ptr(), d["value"].data_ptr(),
                                              d["old_value"].data_ptr() if c["hp"]["clip_value"] else None, d["adv"].data_ptr(),
                                              d["ret"].data_ptr(), d["entropy"].data_ptr(), mask.data_ptr(), n, vd, hp, stats.data_ptr(),
                                              local_n.data_ptr(), _ptr(done), _ptr(trunc), d_new_lp.data_ptr(), d_value.data_ptr(),
                                              d_ent.data_ptr(), terms.data_ptr()), "srl_ppo_loss_fwd_bwd")
    t = terms.cpu().numpy()
    return (dict(d_new_lp=d_new_lp.cpu().numpy(), d_value=d_value.cpu().numpy(), d_entropy=d_ent.cpu().numpy()),
            {k: float(t[i]) for i, k in enumerate(R.LOSS_TERMS)})


def _check_terms(terms, ref, what):
    te = R.loss_term_errors(terms, ref)
    assert te["exact"] == [], (what, te["exact"])
    for k, e in te["sums"].items():
        assert e <= SUM_TOL, (what, k, e)
    for k, e in te["terms"].items():
        assert e <= 4 * LOSS_F32_CPU_ERR[R.TERM_BOUND[k]], (what, k, e)
    lo, hi = te["clip_range"]
    assert lo <= terms["clip"] <= hi, (what, lo, terms["clip"], hi)
    return te


@pytest.mark.parametrize("case", R.LOSS_CASES, ids=_case_id)
def test_ppo_loss_float64(case):
    """The three gradients on every element not near a branch and the ten sums against the float64 restatement, at value_dim 1 and
    3, with local_n the normalisation count or a rank's share of it, the mask as it is and inverted (the trainer's form), done /
    truncated given or NULL.  mask / done / truncated counts are exact; adv / ret are float64 sums of exact terms; the other sums
    are held to the per-element bound of the gradient formed from the same float32 values (loss_ref.TERM_BOUND) times their sum of
    magnitudes, the elements near a branch entering as loss_ref.loss_term_errors derives."""
    c = R.loss_case(*case)
    ref = R.loss_reference(*case)
    cpu = R.loss_reference(*case, torch.float32)
    print("\nfloat32 CPU loss:", R.loss_errors(cpu, ref), R.loss_term_errors(cpu["terms"], ref)["terms"])
    got, terms = _loss_device(c, mask_invert=0, with_done=True)
    for k, g in got.items():
        assert np.isfinite(g).all(), k
    err = R.loss_errors(got, ref)
    te = _check_terms(terms, ref, "mask")
    print("device:", err, te["terms"], te["sums"])
    for k, bound in LOSS_F32_CPU_ERR.items():
        assert err[k] <= 4 * bound, (k, err[k])
    # the trainer's form: the byte is on_reset, the mask its complement; done / truncated NULL leave their sums at 0
    inv, inv_terms = _loss_device(c, mask_invert=1, with_done=False)
    for k in got:
        assert np.array_equal(inv[k].view(np.uint32), got[k].view(np.uint32)), ("mask_invert", k)
    assert inv_terms["done"] == 0.0 and inv_terms["trunc"] == 0.0
    no_done = dict(ref, terms=dict(ref["terms"], done=0.0, trunc=0.0))
    _check_terms(inv_terms, no_done, "inverted mask")
    # (the sums leave each workgroup as atomics, in whatever order the workgroups finish: equal to rounding, bitwise in one workgroup)
    for k in ("policy", "value", "entropy", "clip", "ratio", "adv", "ret", "mask"):
        mag = 0.0 if c["n"] <= 256 or k in ("clip", "mask") else ref["sign_terms"][k] if k in ("adv", "ret") else ref["term_mag"][k]
        assert abs(inv_terms[k] - terms[k]) <= SUM_TOL * mag, ("mask_invert", k)


def test_ppo_loss_argument_errors():
    c = R.loss_case(257, 3, ("smoothl1", 1, 1), "own")
    n, vd = c["n"], c["vd"]
    x, xv = torch.zeros(n, device=DEV), torch.zeros((n, vd), device=DEV)
    mask = torch.ones(n, dtype=torch.uint8, device=DEV)
    stats, local_n = dev(c["norm_stats"], torch.float64), dev(np.array([c["local_n"]]), torch.float64)
    outs = [torch.full((n,), NAN, device=DEV), torch.full((n, vd), NAN, device=DEV), torch.full((n,), NAN, device=DEV)]
    terms = torch.full((hip.LT_COUNT,), 123.0, dtype=torch.float64, device=DEV)

    def call(hp, value_dim=vd, old_value=xv):
        hip._check(hip.lib().srl_ppo_loss_fwd_bwd(hip._stream(), x.data_ptr(), x.data_ptr(), xv.data_ptr(), _ptr(old_value), xv.data_ptr(),
                                                  xv.data_ptr(), x.data_ptr(), mask.data_ptr(), n, value_dim, hp, stats.data_ptr(),
                                                  local_n.data_ptr(), None, None, outs[0].data_ptr(), outs[1].data_ptr(),
                                                  outs[2].data_ptr(), terms.data_ptr()), "srl_ppo_loss_fwd_bwd")

    ok = _hparams(c["hp"], 0)
    bad_kind = _hparams(c["hp"], 0)
    bad_kind.value_loss = 3
    for kw in (dict(hp=bad_kind), dict(hp=ok, value_dim=0), dict(hp=ok, old_value=None)):
        with pytest.raises(hip.HipError):
            call(**kw)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o).all()) for o in outs) and bool((terms == 123.0).all()), "a refused call writes nothing"


# ------------------------------------------------------------------------------------------------ masked statistics / normalisation
NORM_EPS = 1e-5


@pytest.mark.parametrize("n", [1, 257, 2048 * 256 + 3])
def test_masked_stats_and_normalize_float64(n):
    """{count, sum x m, sum (x m)^2} and (x m - mean) / (sqrt(var) + eps) over n elements (the grids are capped at 2048 workgroups:
    the largest n runs the loop's body twice in three threads), x = 3 + 2 randn so that the mean matters, without a mask, with one
    and with the inverted byte, biased and unbiased variance.  The count is exact, the sums are float64 sums of exact terms, and
    the output is the float64 formula rounded once.  The formula takes whatever statistics it is given: the data's own or those of
    a superset (the data-parallel case; the only unbiased form at n = 1, where n / (n - 1) is 1 / 0)."""
    rng = np.random.default_rng(n)
    x2 = (3.0 + 2.0 * rng.standard_normal(2 * n)).astype(np.float32)
    mask2 = (rng.random(2 * n) < 0.7).astype(np.uint8)
    mask2[0] = 1
    x, mask = x2[:n], mask2[:n]
    dx = dev(x)
    L, st = hip.lib(), hip._stream()
    for name, byte, invert in (("none", None, 0), ("mask", mask, 0), ("inverted", 1 - mask, 1)):
        dbyte = None if byte is None else dev(byte, torch.uint8)
        m = None if byte is None else byte.astype(np.float64)
        stats = torch.full((3,), 123.0, dtype=torch.float64, device=DEV)  # overwritten, not accumulated
        hip._check(L.srl_masked_stats(st, dx.data_ptr(), _ptr(dbyte), invert, n, stats.data_ptr()), "srl_masked_stats")
        got = stats.cpu().numpy()
        ref, mag = R.masked_stats(x, m, bool(invert))
        assert got[0] == ref[0], (name, "count")
        assert (np.abs(got[1:] - ref[1:]) <= SUM_TOL * mag[1:]).all(), (name, got, ref)
        superset, _ = R.masked_stats(x2, mask2.astype(np.float64) if byte is not None else None)
        for unbiased in (0, 1):
            for which, s in (("own", ref), ("superset", superset)):
                if unbiased and s[0] < 2:
                    continue
                out = torch.full((n,), NAN, device=DEV)
                ds = dev(s, torch.float64)
                hip._check(L.srl_masked_normalize(st, dx.data_ptr(), _ptr(dbyte), invert, n, ds.data_ptr(), NORM_EPS, unbiased,
                                                  out.data_ptr()), "srl_masked_normalize")
                want = R.masked_normalize(x, m, s, NORM_EPS, bool(unbiased), bool(invert))
                assert within_ulp32(out.cpu().numpy(), want), (name, unbiased, which)
                assert np.array_equal(ds.cpu().numpy(), s), "the statistics are read only"
