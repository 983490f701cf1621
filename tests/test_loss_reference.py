"""The float64 restatements of tests/loss_ref.py that tests/test_gpu_loss_kernels.py holds the HIP kernels to, held in turn against
what they restate -- Philox's known answers, finite differences, the float32 oracle on the golden loss inputs -- and the GPU tests'
own inputs and bounds judged without a GPU: every deliberate fault of the restatements breaks the bound the device is held to,
the exclusions the comparisons use stay below a thousandth, and the inputs reach every branch."""
import numpy as np
import pytest
import torch

import loss_ref as R
from oracle import ppo as oppo
from test_gpu_loss_kernels import CAT_F32_CPU_ERR, LOSS_F32_CPU_ERR, SUM_TOL

CAP = 1e-3       # excluded (row, head) pairs / elements, of all
COVERAGE = 0.01  # of the unmasked elements, per branch
SMALL_CAT = [c for c in R.CAT_CASES if c[0] == 257]
SMALL_LOSS = [c for c in R.LOSS_CASES if c[0] == 257]
_id = lambda c: "-".join("x".join(map(str, v)) if isinstance(v, tuple) else str(v) for v in c)


# ------------------------------------------------------------------------------------------------ the restatements themselves
def test_philox_known_answers():
    """Philox4x32-10's known-answer vectors (Random123's kat_vectors: zeros, all ones, the digits of pi)."""
    words = lambda s: [int(w, 16) for w in s.split()]
    for ctr, key, out in (("00000000 00000000 00000000 00000000", "00000000 00000000", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
                          ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
                          ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1")):
        assert [int(v) for v in R.philox4x32_10(words(ctr), words(key))] == words(out), ctr
    # vectorised over leading dimensions, the key broadcast
    both = R.philox4x32_10(np.array([[0] * 4, [0xffffffff] * 4], np.uint64), np.array([0, 0], np.uint64))
    assert [int(v) for v in both[0]] == words("6627e8d5 e169c58d bc57ac4c 9b00dbd8") and both.shape == (2, 4)


def test_sampler_counter_layout():
    """The counter of (row, head) is {row low, row high, head, offset low} and the key {seed low, seed high}: the uniform the
    sampler uses is the first output word of exactly that block."""
    dims, n = (3, 4), 6
    logits = np.zeros((n, 7), np.float32)
    row0, seed, offset = (3 << 32) + 9, (0xABCDEF01 << 32) | 0x12345678, (7 << 32) + 5
    s = R.categorical_sample(logits, None, None, dims, seed, offset, row0)
    for i in range(n):
        for k, d in enumerate(dims):
            x = int(R.philox4x32_10([(9 + i), 3, k, 5], [0x12345678, 0xABCDEF01])[0])
            assert s["u"][i, k] == (x >> 8) * 2.0**-24 * d and s["action"][i, k] == int((x >> 8) * 2.0**-24 * d)


class _CatFn(torch.autograd.Function):
    """sum(logp d_logp + ent d_ent) of loss_ref.categorical with ITS d_logits as the backward, for gradcheck."""

    @staticmethod
    def forward(ctx, logits, action, avail, dims, d_logp, d_ent):
        with torch.enable_grad():  # the restatement runs its own autograd
            out, _ = R.categorical(logits.detach().numpy(), action, avail, dims, d_logp, d_ent)
        ctx.d_logits = torch.from_numpy(out["d_logits"])
        return torch.tensor((out["logp"] * d_logp + out["ent"] * d_ent).sum())

    @staticmethod
    def backward(ctx, g):
        return g * ctx.d_logits, None, None, None, None, None


def test_categorical_gradient_against_finite_differences():
    """A small masked multi-head case with a head of one action, a head with one available action and a dead head."""
    rng = np.random.default_rng(3)
    dims, n = (3, 1, 4), 6
    logits = 2.0 * rng.standard_normal((n, 8))
    action = np.stack([rng.integers(0, d, n) for d in dims], -1)
    avail = (rng.random((n, 8)) < 0.6)
    avail[np.arange(n)[:, None], np.array([0, 3, 4]) + action] = True
    avail[1, 4:] = False
    avail[1, 4 + action[1, 2]] = True  # one available action
    avail[2, :3] = False               # a dead head
    avail = avail.astype(np.uint8)
    d_logp, d_ent = rng.standard_normal(n), rng.standard_normal(n)
    x = torch.from_numpy(logits).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda t: _CatFn.apply(t, action, avail, dims, d_logp, d_ent), (x,), eps=1e-6, atol=1e-7, rtol=1e-5)
    out, sc = R.categorical(logits, action, avail, dims, d_logp, d_ent)
    assert (out["d_logits"][avail == 0] == 0).all() and (out["d_logits"][2, :3] == 0).all()
    assert out["dead"].sum() == 1 and out["dead"][2, 0] and out["logp_dead"][2] == -np.log(3.0) and out["ent_dead"][2] == np.log(3.0)
    assert (sc["d_logits"][avail == 0] == 0).all() and (sc["d_logits"][avail != 0] > 0).all()


def test_float32_gives_a_dead_head_exactly_zero():
    """What loss_ref.categorical pins a dead head's share to: float32 torch.distributions.Categorical on logits that are all -1e10
    returns log-prob 0 and entropy 0 exactly (float64 returns -log d and log d), and the restatement leaves such a head out."""
    for d in (1, 2, 5, 18):
        dist = torch.distributions.Categorical(logits=torch.full((3, d), R.MASKED_LOGIT, dtype=torch.float32))
        assert (dist.log_prob(torch.tensor([0, d - 1, d // 2])) == 0).all() and (dist.entropy() == 0).all(), d
    logits = np.array([[0.5, -1.0, 2.0, 0.25, 1.0]], np.float32)
    avail = np.array([[0, 0, 0, 1, 1]], np.uint8)
    for dtype in (torch.float32, torch.float64):
        both, sc = R.categorical(logits, np.array([[1, 0]]), avail, (3, 2), dtype=dtype)
        alone, sc1 = R.categorical(logits[:, 3:], np.array([[0]]), avail[:, 3:], (2,), dtype=dtype)
        assert both["logp"] == alone["logp"] and both["ent"] == alone["ent"] and sc["logp"] == sc1["logp"] and sc["ent"] == sc1["ent"]
        assert both["logp_dead"] == -np.log(3.0) and both["ent_dead"] == np.log(3.0)


def test_ppo_loss_float32_is_the_oracle_on_the_golden_inputs(golden):
    """loss_ref.ppo_loss in float32 against oracle.ppo.ppo_loss (itself pinned to the reference's outputs by tests/test_oracle.py) on
    loss.npz's inputs, all eight golden combinations, at that test's tolerances."""
    g = golden("loss.npz")
    flat = lambda k: np.ascontiguousarray(g[k].reshape(-1))
    col = lambda k: np.ascontiguousarray(g[k].reshape(-1, 1))
    inputs = dict(new_lp=flat("new_lp"), old_lp=flat("old_lp"), entropy=flat("entropy"), value=col("value"), old_value=col("old_value"),
                  adv=col("adv"), ret=col("ret"), mask=flat("mask").astype(np.uint8))
    stats = oppo.masked_stats(g["adv"], g["mask"])
    t = lambda k, grad=False: torch.from_numpy(g[k]).clone().requires_grad_(grad)
    for combo in g["combos"]:
        vl, cv, dc = combo.split("_")
        hp = R.loss_hparams((vl, int(cv), int(dc)))
        mine = R.ppo_loss(inputs, hp, stats, stats[0], 0, torch.float32)
        nlp, v, ent = t("new_lp", True), t("value", True), t("entropy", True)
        loss, ostats = oppo.ppo_loss(nlp, t("old_lp"), v, t("old_value"), t("adv"), t("ret"), ent, t("mask"), dual_clip=dc == "1",
                                     value_loss=vl, clip_value=cv == "1", value_loss_config=dict(delta=10.0) if vl == "huber" else {})
        loss.backward()
        tm = mine["terms"]
        m = tm["mask"]
        got = dict(policy_loss=tm["policy"] / m, value_loss=tm["value"] / m, entropy=tm["entropy"] / m, clip_ratio=tm["clip"] / m,
                   importance_weight=tm["ratio"] / m, advantage=tm["adv"] / m, value_targets=tm["ret"] / m)
        total = (tm["policy"] + R._f32(0.5) * tm["value"] - R._f32(0.01) * tm["entropy"]) / m
        assert abs(total - loss.item()) <= 1e-6 * max(1, abs(loss.item())), combo
        for k, val in ostats.items():
            assert abs(got[k] - val) <= 1e-6 * max(1, abs(val)), (combo, k)
        for k, ref in (("d_new_lp", nlp.grad), ("d_value", v.grad), ("d_entropy", ent.grad)):
            assert torch.allclose(torch.from_numpy(mine[k]).float().reshape(ref.shape), ref, rtol=1e-6, atol=1e-9), (combo, k)


def test_masked_normalisation_is_the_oracles(golden):
    g = golden("norm.npz")
    x, mask = g["x"], g["mask"]
    for m, unb in ((mask, False), (None, False), (mask, True)):
        stats, _ = R.masked_stats(x, m)
        assert tuple(stats) == oppo.masked_stats(x, m)
        assert np.array_equal(R.masked_normalize(x, m, stats, 1e-5, unb).astype(np.float32), oppo.masked_normalization(x, m, unbiased=unb))
    inv, _ = R.masked_stats(x, 1.0 - mask, mask_invert=True)
    assert np.array_equal(inv, R.masked_stats(x, mask)[0])


# ------------------------------------------------------------------------------------------------ the GPU tests' inputs and bounds
def _cat_report(case):
    """What the tests below assert about one categorical case, in scalars (the arrays of the large cases are not kept)."""
    n, dims, kind, spread = case
    c = R.cat_case(*case)
    ref, sc = R.cat_reference(*case)
    rep = dict(err=R.categorical_errors(R.cat_reference(*case, torch.float32)[0], ref, sc))
    host = {name: R.sample_rows(c, *args) for name, args in (("5", (R.SAMPLE_SEED, 5)), ("6", (R.SAMPLE_SEED, 6)),
                                                             ("row0", (R.SAMPLE_SEED, 5, R.BIG_ROW0)), ("seed", (R.SAMPLE_SEED_HIGH, 5)))}
    rep["ambiguous"] = {k: float(h["ambiguous"].mean()) for k, h in host.items()}
    rep["forbidden"] = sum(R.sample_forbidden(h["action"], c) for h in host.values())
    sampled = c["is_eval"] == 0
    differs = lambda k: float((host[k]["u"][sampled] != host["5"]["u"][sampled]).mean()) if sampled.any() else 1.0
    rep["other_stream"] = {k: differs(k) for k in ("6", "row0", "seed")}
    if n > R.TAIL:
        tail = R.sample_rows(c, R.SAMPLE_SEED, 5, row0=R.TAIL, start=R.TAIL)
        rep["tail"] = np.array_equal(tail["action"], host["5"]["action"][R.TAIL:]) and np.array_equal(tail["u"], host["5"]["u"][R.TAIL:])
    z = R._masked(c["logits"], c["avail"])
    twice = np.zeros(n, bool)
    for k, s, d in R._heads(dims):
        zk = z[:, s:s + d]
        twice |= ((zk == zk.max(1, keepdims=True)).sum(1) >= 2) & (zk.max(1) > R.MASKED_LOGIT)
    rep["eval_rows_with_a_tie"] = int((twice & ~sampled).sum())
    if c["avail"] is not None:
        one = np.stack([c["avail"][:, s:s + d].sum(1) == 1 for k, s, d in R._heads(dims)], 1)
        rows = one.all(1)  # every head of the row has one available action, the one taken: log 1 and the entropy of a point mass
        rep.update(one=float(one.mean()), point_mass=bool((ref["logp"][rows] == 0).all() and (ref["ent"][rows] == 0).all()))
    rep["dead"] = float(ref["dead"].mean())
    rep["p_min"] = float(np.exp(-(z.max(1) - np.where(z > R.MASKED_LOGIT, z, np.inf).min(1))).min())
    rep["underflow_unmasked"] = int((R.underflowed(c) & (z > R.MASKED_LOGIT)).sum())
    return rep


def _loss_report(case):
    n, vd, combo, form = case
    ref = R.loss_reference(*case)
    cpu = R.loss_reference(*case, torch.float32)
    te = R.loss_term_errors(cpu["terms"], ref)
    unmasked = ref["m"] > 0
    b = ref["branches"]
    cover = dict(b, inside=~b["below"] & ~b["above"])
    return dict(err=R.loss_errors(cpu, ref), te=te, clip=cpu["terms"]["clip"], near=float((ref["near_p"] | ref["near_v"]).mean()),
                cover={k: float(v[unmasked].mean()) for k, v in cover.items()}, masked=float((~unmasked).mean()))


@pytest.fixture(scope="module")
def reports():
    """One pass over the inputs of the GPU tests, shared by the tests below."""
    return dict(cat={c: _cat_report(c) for c in R.CAT_CASES}, loss={c: _loss_report(c) for c in R.LOSS_CASES})


@pytest.mark.parametrize("case", R.CAT_CASES, ids=_id)
def test_categorical_cases_float32_error_and_exclusions(case, reports):
    """On the inputs of the GPU tests: the float32 CPU error the tolerances are four times of stays within a factor of two of what
    is recorded (CPUs differ in the last digits); at most a thousandth of the (row, head) pairs of any sampling call is ambiguous and
    the host sampler itself never picks an unavailable action; another offset, row0 or seed is another stream (the uniforms differ
    on > 99 % of the sampled rows -- the ACTIONS of two streams coincide with probability sum p^2, about a fifth for the 18-way
    head); the tail of a call is the call on the tail with row0; the cases hold what they are for."""
    n, dims, kind, spread = case
    rep = reports["cat"][case]
    print("\nfloat32 CPU Categorical:", rep["err"], "ambiguous:", rep["ambiguous"])
    assert rep["err"]["nonzero_where_exactly_zero"] == 0
    for k, bound in CAT_F32_CPU_ERR.items():
        assert rep["err"][k] <= 2 * bound, (k, rep["err"][k])
    assert max(rep["ambiguous"].values()) <= CAP, rep["ambiguous"]
    assert rep["forbidden"] == 0
    assert rep.get("tail", True)
    if n >= 257:
        assert min(rep["other_stream"].values()) > 0.99, rep["other_stream"]
        assert rep["eval_rows_with_a_tie"] >= 3, "evaluation rows whose maximum is there twice: the pick must be the first"
        if kind in ("single", "dead"):
            assert rep["one"] >= 0.02 and rep["point_mass"]
        assert (rep["dead"] >= 0.02) == (kind == "dead")
    if spread > 2:
        assert rep["p_min"] < 2.0**-24, "probabilities below float32's resolution of 1"
        assert rep["underflow_unmasked"] >= n // 12, "available actions whose float32 exp(z - max) is 0"


@pytest.mark.parametrize("case", R.LOSS_CASES, ids=_id)
def test_loss_cases_float32_error_exclusions_and_coverage(case, reports):
    """On the inputs of the GPU tests: the recorded float32 CPU error (as above); the float32 run's ten sums pass the checks the
    device's are put to; at most a thousandth of the elements is near a branch; and each branch holds at least 1 % of the unmasked
    elements -- ratio below / inside / above the clip, dual clip active, the linear region of Huber / SmoothL1, value clip active
    with either loss winning -- and 1 % of the rows are masked (a single row has one element per channel: from 257 rows on; the
    all-masked-but-one case is exempt from the coverage it exists to lack)."""
    n, vd, combo, form = case
    rep = reports["loss"][case]
    err, te = rep["err"], rep["te"]
    print("\nfloat32 CPU loss:", err, te["terms"], "near a branch:", rep["near"])
    for k, bound in LOSS_F32_CPU_ERR.items():
        assert err[k] <= 2 * bound, (k, err[k])
    assert te["exact"] == [] and all(e <= SUM_TOL for e in te["sums"].values())
    assert all(e <= 4 * LOSS_F32_CPU_ERR[R.TERM_BOUND[k]] for k, e in te["terms"].items()), te["terms"]
    assert te["clip_range"][0] <= rep["clip"] <= te["clip_range"][1]
    assert rep["near"] <= CAP, rep["near"]
    if n >= 257 and form != "one":
        wanted = ["below", "inside", "above"] + ["dual"] * combo[2] + ["linear"] * (combo[0] != "mse") + ["vclip_l1", "vclip_l2"] * combo[1]
        for k in wanted:
            assert rep["cover"][k] >= COVERAGE, (k, rep["cover"][k])
        assert rep["masked"] >= COVERAGE


def test_recorded_float32_errors_are_the_measured_ones(reports):
    """The maxima over all cases are no less than half the recorded constants: a constant far above what is measured would be a
    loose tolerance."""
    worst_cat = {k: max(r["err"][k] for r in reports["cat"].values()) for k in CAT_F32_CPU_ERR}
    worst_loss = {k: max(r["err"][k] for r in reports["loss"].values()) for k in LOSS_F32_CPU_ERR}
    print("\nfloat32 CPU, maxima:", worst_cat, worst_loss)
    flagged = sum(r["near"] > 0 for c, r in reports["loss"].items() if c[0] > 1000)
    assert flagged >= 6, "the large cases keep the elements the exclusion is for"
    for k, bound in CAT_F32_CPU_ERR.items():
        assert 0.5 * bound <= worst_cat[k], (k, worst_cat[k])
    for k, bound in LOSS_F32_CPU_ERR.items():
        assert 0.5 * bound <= worst_loss[k], (k, worst_loss[k])


# ------------------------------------------------------------------------------------------------ the tolerances can fail
def _breaks_cat(got, ref, sc):
    err = R.categorical_errors(got, ref, sc)
    if err.get("nonzero_where_exactly_zero"):
        return float("inf")
    return max(err[k] / (4 * b) for k, b in CAT_F32_CPU_ERR.items() if k in err)


@pytest.mark.parametrize("case", SMALL_CAT, ids=_id)
def test_categorical_tolerances_can_fail(case):
    """Each fault of the float64 restatement, on the 257-row inputs of the GPU tests, fails the comparison the device has to pass:
    the entropy's gradient with the wrong sign; gradient reaching overwritten logits (visible where a masked action has
    probability: the dead heads); one draw shared by all heads; row0 left out of the counter; the CDF over the unmasked logits."""
    n, dims, kind, spread = case
    c = R.cat_case(*case)
    ref, sc = R.cat_reference(*case)
    run = lambda fault: R.categorical(c["logits"], c["action"], c["avail"], dims, c["d_logp"], c["d_ent"], fault=fault)[0]
    assert _breaks_cat(run(None), ref, sc) == 0.0
    if max(dims) >= 2:
        assert _breaks_cat(run("entropy_grad_sign"), ref, sc) > 10
    if kind == "dead":
        assert _breaks_cat(run("masked_gets_gradient"), ref, sc) == float("inf")
    host = R.sample_rows(c, R.SAMPLE_SEED, 5)
    if len(dims) > 1:
        assert R.sample_mismatches(R.sample_rows(c, R.SAMPLE_SEED, 5, fault="heads_share_draw")["action"], host) > 0
    far = R.sample_rows(c, R.SAMPLE_SEED, 5, row0=R.BIG_ROW0)
    assert R.sample_mismatches(R.sample_rows(c, R.SAMPLE_SEED, 5, row0=R.BIG_ROW0, fault="row0_ignored")["action"], far) > 0
    if c["avail"] is not None:
        bad = R.sample_rows(c, R.SAMPLE_SEED, 5, fault="picks_unavailable")["action"]
        assert R.sample_forbidden(bad, c) > 0 and R.sample_mismatches(bad, host) > 0
    # a sampler that drops the offset's word, or either word of the seed, does not follow the host either
    assert R.sample_mismatches(R.sample_rows(c, R.SAMPLE_SEED, 6)["action"], host) > 0
    assert R.sample_mismatches(R.sample_rows(c, R.SAMPLE_SEED_HIGH & 0xFFFFFFFF, 5)["action"], R.sample_rows(c, R.SAMPLE_SEED_HIGH, 5)) > 0


def _breaks_loss(bad, ref):
    if not all(np.isfinite(bad[k]).all() for k in LOSS_F32_CPU_ERR):
        return float("inf")
    err = R.loss_errors(bad, ref)
    te = R.loss_term_errors(bad["terms"], ref)
    worst = max(err[k] / (4 * b) for k, b in LOSS_F32_CPU_ERR.items())
    worst = max([worst] + [e / (4 * LOSS_F32_CPU_ERR[R.TERM_BOUND[k]]) for k, e in te["terms"].items()])
    worst = max([worst] + [e / SUM_TOL for e in te["sums"].values()])
    return float("inf") if te["exact"] or not te["clip_range"][0] <= bad["terms"]["clip"] <= te["clip_range"][1] else worst


@pytest.mark.parametrize("case", SMALL_LOSS, ids=_id)
def test_loss_tolerances_can_fail(case):
    """Each fault of the float64 restatement, on the 257-row inputs of the GPU tests and wherever it applies, fails the comparison
    the device has to pass: masked means over rows x channels (value_dim 3); the inverted byte taken as the mask; the quadratic's
    slope past delta (Huber / SmoothL1); no dual clip; local_n as the normalisation count (a rank's share)."""
    n, vd, combo, form = case
    c = R.loss_case(*case)
    ref = R.loss_reference(*case)
    run = lambda fault, inputs=c["inputs"], inv=0: R.ppo_loss(inputs, c["hp"], c["norm_stats"], c["local_n"], inv, fault=fault)
    assert _breaks_loss(run(None), ref) == 0.0
    inverted = dict(c["inputs"], mask=1 - c["inputs"]["mask"])
    assert _breaks_loss(run(None, inverted, 1), ref) == 0.0
    assert _breaks_loss(run("mask_not_inverted", inverted, 1), ref) > 10
    if vd > 1:
        assert _breaks_loss(run("mean_over_channels"), ref) > 10
    reached = lambda k: bool(ref["branches"][k][ref["m"] > 0].any())  # (the all-masked-but-one case has one row to reach with)
    if combo[0] != "mse" and reached("linear"):
        assert _breaks_loss(run("huber_linear_slope"), ref) > 10
    if combo[2] and reached("dual"):
        assert _breaks_loss(run("dual_clip_off"), ref) > 10
    if form != "own":
        assert _breaks_loss(run("norm_by_local_n"), ref) > 10
