"""GPU parity tests, kernel by kernel, through the C ABI (ctypes binding ``srl_amd.hip``).

Each kernel is compared with the CPU oracle (``oracle/``) on the same seeded inputs and with the golden
vectors generated from the real reference (``tests/golden/*.npz``).  Tolerances: GAE returns and PPO loss
1e-5 relative (the bar BASELINE.json states); network pieces are float32 MFMA chains checked at 1e-5
relative to the scale of the output (float64-referenced where cheap).
"""
import os

import numpy as np
import pytest
import torch

from oracle import gae as ogae
from oracle import ppo as oppo
from srl_amd import hip
from srl_amd.algorithm.rnnpath import CELLS, bufs_of
from srl_amd.runtime import synthetic

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


needs_f16x2 = pytest.mark.skipif(__import__("os").environ.get("SRL_F16X2", "1")[:1] == "0",
                                 reason="a test OF the two-piece f16 kernels, which SRL_F16X2=0 switches off")


def rel_close(a, b, rtol=1e-5, scale=None):
    """|a-b| <= rtol * max(|b|, scale): the tolerance form of SURVEY.md section 7."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = float(np.abs(b).max()) if scale is None else scale
    return bool((np.abs(a - b) <= rtol * np.maximum(np.abs(b), max(scale, 1e-30))).all())


def dev(x, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(x))
    if dtype is not None:
        t = t.to(dtype)
    return t.to(DEV).contiguous()


def run_gae(arr, gamma, lmbda, ratio=None):
    Tb, B = arr["on_reset"].shape[:2]
    Nc = arr["value"].shape[2]
    adv = torch.full((Tb, B, Nc), 7.0, device=DEV)
    ret = torch.full((Tb, B, Nc), 7.0, device=DEV)
    stats = torch.full((3,), -1.0, dtype=torch.float64, device=DEV)
    hip.gae_scan(dev(arr["reward"]), dev(arr["value"]), dev(arr["done"]), dev(arr["truncated"]), dev(arr["on_reset"]),
                 gamma, lmbda, adv, ret, stats=stats, imp_ratio=None if ratio is None else dev(ratio))
    torch.cuda.synchronize()
    return adv.cpu().numpy(), ret.cpu().numpy(), stats.cpu().numpy()


# ------------------------------------------------------------------------------------------------ GAE
def test_gae_golden_cases(golden):
    g = golden("gae.npz")
    for name in g["cases"]:
        arr = {k: g[f"{name}_{k}"] for k in ("reward", "value", "done", "truncated", "on_reset")}
        for tag, gam, lam in (("a", 0.99, 0.97), ("b", 0.9, 0.5)):
            adv, ret, stats = run_gae(arr, gam, lam)
            ref_adv, ref_ret = g[f"{name}_{tag}_adv"], g[f"{name}_{tag}_ret"]
            T = ref_adv.shape[0]
            assert rel_close(adv[:T], ref_adv, 1e-5, scale=1.0), (name, tag)
            assert rel_close(ret[:T], ref_ret, 1e-5, scale=1.0), (name, tag)
            assert (adv[T:] == 7.0).all() and (ret[T:] == 7.0).all()  # the pad row is the caller's
            mask = 1.0 - arr["on_reset"][1:].astype(np.float64)
            n, s, q = oppo.masked_stats(ref_adv, mask)  # [T, B, 1] mask: counted once, sums over all value channels
            assert stats[0] == n
            assert abs(stats[1] - s) <= 1e-5 * max(1.0, q**0.5) and abs(stats[2] - q) <= 1e-6 * max(1, q)
        adv, _, _ = run_gae(arr, 0.99, 0.97, ratio=g[f"{name}_ratio"])
        assert rel_close(adv[:T], g[f"{name}_vtrace_adv"], 1e-5, scale=1.0), (name, "vtrace")


def test_gae_hand_case(golden):
    """The hand-computed vector of the reference's own test (legacy/tests/modules_test.py:119-138)."""
    g = golden("gae.npz")
    shp = lambda x: x.reshape(-1, 1, 1)
    arr = dict(reward=shp(g["hand_reward"]), value=shp(g["hand_value"]), done=shp(g["hand_done"]).astype(np.uint8),
               truncated=shp(g["hand_truncated"]).astype(np.uint8), on_reset=shp(g["hand_on_reset"]).astype(np.uint8))
    adv, _, _ = run_gae(arr, 0.1, 0.1)
    expect = np.array([2.1 * 0.01 - 1, 2.1, 0, -0.8 + 0.01, 1, 0, 0.111, 1.1])
    keep = 1 - g["hand_on_reset"][1:]
    np.testing.assert_array_almost_equal(adv[:8, 0, 0] * keep, expect * keep)
    # note: the reference's value at done is NOT pre-masked in this test; the kernel masks value by done itself


@pytest.mark.parametrize("T,B,Nc", [(1, 1, 1), (2, 3, 1), (128, 512, 1), (400, 37, 1), (130, 70, 2), (1000, 9, 1),
                                    (16, 40000, 1), (1000, 12, 1), (300, 33000, 1), (77, 36864, 1), (5, 8, 1),
                                    (64, 4, 1), (257, 256, 1), (40, 131072, 1), (6, 400000, 1)])
def test_gae_shapes_vs_oracle(T, B, Nc):
    # B % 4 == 0 with one value channel takes the register-resident kernel (64- or 128-byte rows,
    # 1/2/4 time rows per lane, several time tiles when T is long); everything else the LDS-tile one
    arr = synthetic.make_sample_arrays(seed=T + B, T=T, B=B, obs_spec={}, action_dims=2, p_done=0.03, value_dim=Nc)
    a = dict(reward=arr["reward"], value=arr["analyzed_result.value"], done=arr["done"], truncated=arr["truncated"],
             on_reset=arr["on_reset"])
    adv, ret, stats = run_gae(a, 0.99, 0.97)
    o_adv, o_ret = ogae.adv_and_value_target(a["reward"], a["value"], a["truncated"], a["done"], a["on_reset"], 0.99,
                                             0.97)
    if Nc == 1:  # V-trace through the same tiling
        ratio = np.random.RandomState(T).uniform(0.3, 1.8, size=(T, B, 1)).astype(np.float32)
        vadv, _, _ = run_gae(a, 0.99, 0.97, ratio=ratio)
        o_vadv, _ = ogae.adv_and_value_target(a["reward"], a["value"], a["truncated"], a["done"], a["on_reset"], 0.99,
                                              0.97, vtrace=True, imp_ratio=ratio)
        assert rel_close(vadv[:T], o_vadv, 1e-5, scale=1.0)
    assert rel_close(adv[:T], o_adv, 1e-5, scale=1.0)
    assert rel_close(ret[:T], o_ret, 1e-5, scale=1.0)
    # the mask is [T, B, 1]: its sum counts every (step, env) once, the value sums run over all channels (utils.py:41-55)
    n, s, q = oppo.masked_stats(o_adv, 1.0 - a["on_reset"][1:].astype(np.float64))
    assert stats[0] == n and abs(stats[1] - s) <= 1e-6 * max(1.0, abs(s), q**0.5) and abs(stats[2] - q) <= 1e-6 * q + 1e-9


def test_gae_tensor_gamma_lambda_golden(golden):
    """gamma / lmbda as [T, B, 1] float32 tensors (reference gae.py:51-60) against the reference's own outputs."""
    g = golden("gae_tensor.npz")
    for name in g["cases"]:
        arr = {k: g[f"{name}_{k}"] for k in ("reward", "value", "done", "truncated", "on_reset")}
        gam, lam = dev(g[f"{name}_gamma"]), dev(g[f"{name}_lambda"])
        for tag, gg, ll in (("gl", gam, lam), ("g", gam, 0.95), ("l", 0.99, lam)):
            adv, ret, _ = run_gae(arr, gg, ll)
            ref = g[f"{name}_{tag}_adv"]
            T = ref.shape[0]
            assert rel_close(adv[:T], ref, 1e-5, scale=1.0), (name, tag)
            vm = (arr["value"] * (1 - arr["done"])).astype(np.float32)
            assert rel_close(ret[:T], ref + vm[:T], 1e-5, scale=1.0), (name, tag)
        adv, _, _ = run_gae(arr, gam, lam, ratio=g[f"{name}_ratio"])
        assert rel_close(adv[:T], g[f"{name}_vtrace_adv"], 1e-5, scale=1.0), (name, "vtrace")
    with pytest.raises(hip.HipError):  # a tensor of the wrong shape is refused like the reference's assert (gae.py:53)
        run_gae(arr, gam[:-1], 0.9)


@pytest.mark.parametrize("T,B", [(128, 4096), (128, 512), (33, 12), (64, 90000), (7, 10)])
def test_gae_stats_workspace_is_reproducible_and_self_resetting(T, B):
    """With a workspace the three sums need no zeroing launch: partial sums per workgroup, added in workgroup order by the
    last workgroup to finish.  Same sums as the atomic path (to float64 rounding), bitwise equal from launch to launch, and
    the workspace is ready for the next launch without the caller touching it."""
    arr = synthetic.make_sample_arrays(seed=3 * T + B, T=T, B=B, obs_spec={}, action_dims=2, p_done=0.03)
    a = [dev(arr[k]) for k in ("reward", "analyzed_result.value", "done", "truncated", "on_reset")]
    adv, ret = torch.zeros((T + 1, B, 1), device=DEV), torch.zeros((T + 1, B, 1), device=DEV)
    ws = hip.gae_scan_workspace(B, 1, DEV)
    ref = torch.zeros(3, dtype=torch.float64, device=DEV)
    hip.gae_scan(*a, 0.99, 0.97, adv, ret, stats=ref)
    adv_ref = adv.clone()
    outs = []
    for _ in range(4):
        st = torch.full((3,), 123.0, dtype=torch.float64, device=DEV)  # overwritten, not accumulated
        hip.gae_scan(*a, 0.99, 0.97, adv, ret, stats=st, workspace=ws)
        outs.append(st.cpu().numpy())
    assert torch.equal(adv, adv_ref)
    r = ref.cpu().numpy()
    assert outs[0][0] == r[0] and np.allclose(outs[0], r, rtol=1e-12, atol=1e-9)
    assert all(np.array_equal(o, outs[0]) for o in outs[1:])
    assert int(ws.view(torch.int32)[0].item()) == 0  # the ticket is back at zero


def test_gae_empty():
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=DEV)
    stats = torch.ones(3, dtype=torch.float64, device=DEV)
    hip.gae_scan(z(1, 0, 1), z(1, 0, 1), z(1, 0, 1, dt=torch.uint8), z(1, 0, 1, dt=torch.uint8),
                 z(1, 0, 1, dt=torch.uint8), 0.99, 0.97, z(1, 0, 1), z(1, 0, 1), stats=stats)
    assert (stats.cpu().numpy() == 0).all()


# ------------------------------------------------------------------------------------------------ normalisation
def test_masked_normalize_golden(golden):
    g = golden("norm.npz")
    x, mask = g["x"], g["mask"]
    for tag, m, unb in (("masked", mask, False), ("nomask", None, False), ("unbiased", mask, True)):
        stats = torch.zeros(3, dtype=torch.float64, device=DEV)
        md = None if m is None else dev(m, torch.uint8)
        hip.masked_stats(dev(x), md, stats)
        assert np.allclose(stats.cpu().numpy(), g[f"{tag}_stats"], rtol=1e-12)
        out = torch.empty(x.shape, device=DEV)
        hip.masked_normalize(dev(x), md, stats, out, unbiased=unb)
        assert rel_close(out.cpu().numpy(), g[f"{tag}_out"], 1e-5, scale=1.0), tag
    # inverted-byte form (mask = 1 - on_reset)
    stats = torch.zeros(3, dtype=torch.float64, device=DEV)
    hip.masked_stats(dev(x), dev(1 - mask, torch.uint8), stats, mask_invert=True)
    assert np.allclose(stats.cpu().numpy(), g["masked_stats"], rtol=1e-12)


# ------------------------------------------------------------------------------------------------ PPO loss
def _hp(vl, cv, dc, **kw):
    base = dict(eps_clip=0.2, c_clip=3.0, value_eps_clip=0.2, value_loss_weight=0.5, entropy_bonus_weight=0.01,
                huber_delta=10.0 if vl == "huber" else 1.0, norm_eps=1e-5, dual_clip=int(dc), clip_value=int(cv),
                value_loss=hip.VALUE_LOSS_KINDS[vl], mask_invert=0)
    base.update(kw)
    return hip.PpoHparams(**base)


def run_loss(inp, hp):
    n = inp["new_lp"].size
    f = lambda k: dev(inp[k]).reshape(-1)
    mask = dev(inp["mask"], torch.uint8).reshape(-1)
    stats = torch.zeros(3, dtype=torch.float64, device=DEV)
    hip.masked_stats(f("adv"), mask, stats)
    outs = [torch.empty(n, device=DEV) for _ in range(3)]
    terms = torch.empty(hip.LT_COUNT, dtype=torch.float64, device=DEV)
    hip.ppo_loss_fwd_bwd(f("new_lp"), f("old_lp"), f("value"), f("old_value"), f("adv"), f("ret"), f("entropy"), mask, hp,
                         stats, stats[0:1], *outs, terms)
    t = terms.cpu().numpy()
    m = t[hip.LT_MASK]
    loss = (t[hip.LT_POLICY] + hp.value_loss_weight * t[hip.LT_VALUE] - hp.entropy_bonus_weight * t[hip.LT_ENTROPY]) / m
    stats_out = dict(loss=loss, policy_loss=t[hip.LT_POLICY] / m, value_loss=t[hip.LT_VALUE] / m,
                     entropy=t[hip.LT_ENTROPY] / m, clip_ratio=t[hip.LT_CLIP] / m, importance_weight=t[hip.LT_RATIO] / m,
                     advantage=t[hip.LT_ADV] / m, value_targets=t[hip.LT_RET] / m)
    return stats_out, [o.cpu().numpy().reshape(inp["new_lp"].shape) for o in outs]


def test_ppo_loss_golden(golden):
    g = golden("loss.npz")
    inp = {k: g[k] for k in ("new_lp", "old_lp", "value", "old_value", "adv", "ret", "entropy", "mask")}
    names = list(g["stat_names"])
    for combo in g["combos"]:
        vl, cv, dc = combo.split("_")
        stats, grads = run_loss(inp, _hp(vl, cv == "1", dc == "1"))
        ref = dict(zip(names, g[f"{combo}_stats"]))
        for k, v in ref.items():
            assert abs(stats[k] - v) <= 1e-5 * max(abs(v), 1e-3), (combo, k, stats[k], v)
        for got, key in zip(grads, ("d_new_lp", "d_value", "d_entropy")):
            assert rel_close(got, g[f"{combo}_{key}"], 1e-5), (combo, key)


def test_ppo_loss_vs_oracle_large():
    rng = np.random.default_rng(0)
    shape = (128, 300, 1)
    inp = dict(new_lp=-1 + 0.4 * rng.standard_normal(shape), old_lp=-1 + 0.4 * rng.standard_normal(shape),
               value=rng.standard_normal(shape), old_value=rng.standard_normal(shape), adv=3 * rng.standard_normal(shape),
               ret=2 * rng.standard_normal(shape), entropy=1 + 0.1 * rng.standard_normal(shape),
               mask=(rng.random(shape) < 0.9))
    inp = {k: v.astype(np.float32) for k, v in inp.items()}
    for vl, cv, dc in (("mse", False, True), ("huber", True, False), ("smoothl1", True, True)):
        stats, grads = run_loss(inp, _hp(vl, cv, dc))
        t = lambda k, g=False: torch.from_numpy(inp[k]).clone().requires_grad_(g)
        nlp, v, ent = t("new_lp", True), t("value", True), t("entropy", True)
        loss, ostats = oppo.ppo_loss(nlp, t("old_lp"), v, t("old_value"), t("adv"), t("ret"), ent, t("mask"),
                                     dual_clip=dc, value_loss=vl, clip_value=cv,
                                     value_loss_config=dict(delta=10.0) if vl == "huber" else {})
        loss.backward()
        assert abs(stats["loss"] - loss.item()) <= 1e-5 * abs(loss.item())
        for k, val in ostats.items():
            assert abs(stats[k] - val) <= 1e-5 * max(abs(val), 1e-3), (vl, k)
        for got, ref in zip(grads, (nlp.grad, v.grad, ent.grad)):
            assert rel_close(got, ref.numpy(), 1e-5), vl


# ------------------------------------------------------------------------------------------------ categorical
def _cat_ref(logits, action, dims, avail=None):
    lg = torch.from_numpy(logits).clone().requires_grad_(True)
    x = lg if avail is None else lg.masked_fill(torch.from_numpy(avail) == 0, -1e10)
    lp, ent, s = 0, 0, 0
    for k, d in enumerate(dims):
        dist = torch.distributions.Categorical(logits=x[:, s:s + d])
        lp = lp + dist.log_prob(torch.from_numpy(action[:, k]).long())
        ent = ent + dist.entropy()
        s += d
    return lg, lp, ent


@pytest.mark.parametrize("dims,use_avail", [([2], False), ([6], False), ([3, 4], False), ([9], True), ([18], False)])
def test_categorical_fwd_bwd(dims, use_avail):
    rng = np.random.default_rng(1)
    n, atot = 1000, sum(dims)
    logits = (2 * rng.standard_normal((n, atot))).astype(np.float32)
    action = np.stack([rng.integers(0, d, n) for d in dims], -1).astype(np.int32)
    avail = None
    if use_avail:
        avail = (rng.random((n, atot)) < 0.6)
        avail[np.arange(n), action[:, 0]] = True
        avail = avail.astype(np.uint8)
    lp = torch.empty(n, device=DEV)
    ent = torch.empty(n, device=DEV)
    av = None if avail is None else dev(avail)
    hip.categorical_fwd(dev(logits), dev(action), av, dims, lp, ent)
    lg, rlp, rent = _cat_ref(logits, action, dims, avail)
    assert rel_close(lp.cpu().numpy(), rlp.detach().numpy(), 1e-5, scale=1.0)
    assert rel_close(ent.cpu().numpy(), rent.detach().numpy(), 1e-5, scale=1.0)
    glp = rng.standard_normal(n).astype(np.float32)
    gent = rng.standard_normal(n).astype(np.float32)
    (rlp * torch.from_numpy(glp) + rent * torch.from_numpy(gent)).sum().backward()
    dl = torch.empty((n, atot), device=DEV)
    hip.categorical_bwd(dev(logits), dev(action), av, dims, dev(glp), dev(gent), dl)
    assert rel_close(dl.cpu().numpy(), lg.grad.numpy(), 2e-5, scale=1.0)


def test_categorical_sample_distribution_and_eval():
    dims = [5]
    n = 200000
    logits = np.tile(np.log(np.array([0.1, 0.2, 0.3, 0.25, 0.15], np.float32)), (n, 1))
    is_eval = np.zeros(n, np.uint8)
    is_eval[:100] = 1
    act = torch.empty((n, 1), dtype=torch.int64, device=DEV)
    lp = torch.empty((n, 1), device=DEV)
    hip.categorical_sample(dev(logits), None, dev(is_eval), dims, 123, 0, act, lp)
    a = act.cpu().numpy()[:, 0]
    assert (a[:100] == 2).all()  # argmax rows
    freq = np.bincount(a[100:], minlength=5) / (n - 100)
    assert np.abs(freq - np.array([0.1, 0.2, 0.3, 0.25, 0.15])).max() < 5e-3
    assert np.allclose(lp.cpu().numpy()[:, 0], logits[np.arange(n), a], atol=1e-5)
    # same (seed, offset) -> same stream; different offset -> different stream
    act2 = torch.empty_like(act)
    hip.categorical_sample(dev(logits), None, dev(is_eval), dims, 123, 0, act2, lp)
    assert torch.equal(act, act2)
    hip.categorical_sample(dev(logits), None, dev(is_eval), dims, 123, 1, act2, lp)
    assert not torch.equal(act, act2)


# ------------------------------------------------------------------------------------------------ GEMM
def _gemm_ref(A, B, akm, bkm):
    A64 = A.astype(np.float64).T if akm else A.astype(np.float64)
    B64 = B.astype(np.float64) if bkm else B.astype(np.float64).T
    return A64 @ B64


@pytest.mark.parametrize("M,N,K", [(256, 64, 64), (1000, 2, 64), (300, 64, 4), (513, 130, 77), (64, 512, 3136),
                                   (4096, 32, 256), (130, 7, 512), (33, 300, 50)])
@pytest.mark.parametrize("akm,bkm", [(0, 0), (0, 1), (1, 1)])
def test_gemm_orientations(M, N, K, akm, bkm):
    rng = np.random.default_rng(M + N + K)
    A = rng.standard_normal((K, M) if akm else (M, K)).astype(np.float32)
    B = rng.standard_normal((K, N) if bkm else (N, K)).astype(np.float32)
    C = torch.full((M, N), np.nan, device=DEV)
    dA, dB = dev(A), dev(B)
    hip.gemm(M, N, K, dA.data_ptr(), A.shape[1], akm, dB.data_ptr(), B.shape[1], bkm, C.data_ptr(), N)
    ref = _gemm_ref(A, B, akm, bkm)
    assert rel_close(C.cpu().numpy(), ref, 1e-5, scale=float(np.sqrt(K)))


@pytest.mark.parametrize("akm,bkm", [(0, 0), (0, 1), (1, 1), (1, 0)])
@pytest.mark.parametrize("M,N,K,dyn", [(512, 384, 1024, 0), (260, 200, 3136, 0), (1024, 128, 512, 12), (384, 640, 2048, 30)])
def test_gemm_bf16x3_is_as_accurate_as_the_float32_mfma(M, N, K, dyn, akm, bkm):
    """float32 GEMMs run on the bf16 matrix cores with three exact bf16 pieces per operand and the six leading piece
    products (gemm_bf16x3.h).  Against float64: the error must be that of a float32 contraction -- compared here with the
    float32-MFMA kernel (SRL_MFMA=f32) on the same inputs, element by element and in the mean.  `dyn`: operands spread over
    2^+-dyn in magnitude (every piece keeps float32's exponent range: no scaling, no underflow)."""
    import os
    rng = np.random.default_rng(M + N + K + dyn)
    spread = lambda shape: (rng.standard_normal(shape) * np.exp2(rng.uniform(-dyn, dyn, shape))).astype(np.float32)
    A, B = spread((K, M) if akm else (M, K)), spread((K, N) if bkm else (N, K))
    dA, dB = dev(A), dev(B)
    ref = _gemm_ref(A, B, akm, bkm)
    A64 = np.abs(A.astype(np.float64).T if akm else A.astype(np.float64))
    B64 = np.abs(B.astype(np.float64) if bkm else B.astype(np.float64).T)
    mag = A64 @ B64  # sum_k |a||b|: the scale rounding errors are relative to
    errs = {}
    for mode in ("bf16x3", "f32"):
        if mode == "f32":
            os.environ["SRL_MFMA"] = "f32"
        try:
            C = torch.full((M, N), np.nan, device=DEV)
            hip.gemm(M, N, K, dA.data_ptr(), A.shape[1], akm, dB.data_ptr(), B.shape[1], bkm, C.data_ptr(), N)
            errs[mode] = np.abs(C.cpu().numpy().astype(np.float64) - ref) / mag
        finally:
            os.environ.pop("SRL_MFMA", None)
    # float32 unit roundoff is 6e-8; a K-term float32 sum stays well below K times that
    assert errs["bf16x3"].max() <= 2e-6 and errs["f32"].max() <= 2e-6, (errs["bf16x3"].max(), errs["f32"].max())
    assert errs["bf16x3"].mean() <= 1.5 * errs["f32"].mean() + 1e-9, (errs["bf16x3"].mean(), errs["f32"].mean())
    assert errs["bf16x3"].max() <= 3.0 * errs["f32"].max() + 1e-9, (errs["bf16x3"].max(), errs["f32"].max())


@needs_f16x2
@pytest.mark.parametrize("kind", ["normal", "relu-x-small-w", "wide-range"])
@pytest.mark.parametrize("M,N,K", [(512, 384, 1024), (260, 200, 3136), (16384, 512, 576)])
def test_gemm_f16x2_forward_is_as_accurate_as_the_float32_mfma(M, N, K, kind):
    """Forward products whose caller hands over both operands' ranges run on TWO f16 pieces per operand and three piece
    products (gemm_bf16x3.h, NP == 2).  Same gate as the three-plane bf16 kernel: against float64, no worse than 1.5x in the
    mean and 3x at the maximum than the float32-MFMA kernel on the same inputs -- for the operands it is meant for: weights
    (small, narrow range) and ReLU'd / LayerNorm'd activations, and for operands spread over 2^+-8.  The ranges come from
    srl_absmax; without them the same call takes the three-plane kernel (operands of unknown dynamic range: the `dyn`
    cases of the test above never see this kernel)."""
    import os
    rng = np.random.default_rng(M + N + K)
    if kind == "normal":
        A, B = rng.standard_normal((M, K)), rng.standard_normal((N, K))
    elif kind == "relu-x-small-w":  # activations after a ReLU (half zeros, a long tail) against weights ~ 1 / sqrt(K)
        A = np.maximum(rng.standard_normal((M, K)) * 3.0, 0.0)
        B = rng.standard_normal((N, K)) / np.sqrt(K)
    else:
        A = rng.standard_normal((M, K)) * np.exp2(rng.uniform(-8, 8, (M, K)))
        B = rng.standard_normal((N, K)) * np.exp2(rng.uniform(-8, 8, (N, K)))
    A, B = A.astype(np.float32), B.astype(np.float32)
    dA, dB = dev(A), dev(B)
    ref = A.astype(np.float64) @ B.astype(np.float64).T
    mag = np.abs(A.astype(np.float64)) @ np.abs(B.astype(np.float64)).T
    rng_ab = torch.zeros(3, device=DEV)
    hip.absmax(dA.data_ptr(), A.size, rng_ab.data_ptr())
    hip.absmax(dB.data_ptr(), B.size, rng_ab.data_ptr() + 4)
    assert rng_ab[:2].cpu().tolist() == [float(np.abs(A).max()), float(np.abs(B).max())]
    errs, counts = {}, {}
    for mode in ("f16x2", "bf16x3", "f32"):
        if mode == "f32":
            os.environ["SRL_MFMA"] = "f32"
        try:
            C = torch.full((M, N), np.nan, device=DEV)
            hip.dispatch_counts(reset=True)
            kw = dict(a_absmax=rng_ab.data_ptr(), b_absmax=rng_ab.data_ptr() + 4, out_absmax=rng_ab.data_ptr() + 8) if mode == "f16x2" else {}
            hip.gemm(M, N, K, dA.data_ptr(), K, 0, dB.data_ptr(), K, 0, C.data_ptr(), N, **kw)
            counts[mode] = hip.dispatch_counts(reset=True)
            out = C.cpu().numpy()
            errs[mode] = np.abs(out.astype(np.float64) - ref) / mag.clip(1e-30)
            if mode == "f16x2":
                assert float(rng_ab[2]) == float(np.abs(out).max())  # the epilogue's range of the result
        finally:
            os.environ.pop("SRL_MFMA", None)
    assert counts["f16x2"]["gemm2h"] == 1 and counts["bf16x3"]["gemm3"] == 1 and counts["f32"]["gemm_f32"] == 1, counts
    assert errs["f16x2"].max() <= 2e-6, errs["f16x2"].max()
    assert errs["f16x2"].mean() <= 1.5 * errs["f32"].mean() + 1e-9, (errs["f16x2"].mean(), errs["f32"].mean(), errs["bf16x3"].mean())
    assert errs["f16x2"].max() <= 3.0 * errs["f32"].max() + 1e-9, (errs["f16x2"].max(), errs["f32"].max(), errs["bf16x3"].max())


def test_gemm_epilogues_and_split():
    rng = np.random.default_rng(5)
    M, N, K = 700, 96, 200
    A = rng.standard_normal((M, K)).astype(np.float32)
    W = rng.standard_normal((N, K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    dA, dW, db = dev(A), dev(W), dev(b)
    for act, fn in ((1, lambda z: np.maximum(z, 0)), (2, np.tanh)):
        C = torch.empty((M, N), device=DEV)
        hip.gemm(M, N, K, dA.data_ptr(), K, 0, dW.data_ptr(), K, 0, C.data_ptr(), N, bias=db.data_ptr(), act=act)
        ref = fn(A.astype(np.float64) @ W.astype(np.float64).T + b)
        if act == 1:
            assert rel_close(C.cpu().numpy(), ref, 1e-5, scale=float(np.sqrt(K)))
        else:  # |tanh'| <= 1: the pre-activation error bound carries over as an absolute bound
            assert np.abs(C.cpu().numpy() - ref).max() <= 1e-5 * np.sqrt(K)
    # dgrad with the activation mask of the producer, accumulated on top of existing contents
    Y = np.maximum(rng.standard_normal((M, K)), 0).astype(np.float32)
    dZ = rng.standard_normal((M, N)).astype(np.float32)
    base = rng.standard_normal((M, K)).astype(np.float32)
    C = dev(base).clone()
    dY, ddZ = dev(Y), dev(dZ)
    hip.gemm(M, K, N, ddZ.data_ptr(), N, 0, dW.data_ptr(), K, 1, C.data_ptr(), K, dact_src=dY.data_ptr(), ld_dact=K,
             dact=1, accumulate=True)
    ref = base + (dZ.astype(np.float64) @ W.astype(np.float64)) * (Y > 0)
    assert rel_close(C.cpu().numpy(), ref, 1e-5, scale=float(np.sqrt(N)))
    # weight gradient with split-K through a workspace, accumulated
    rows = 50000
    dZ = rng.standard_normal((rows, 40)).astype(np.float32)
    X = rng.standard_normal((rows, 72)).astype(np.float32)
    g0 = rng.standard_normal((40, 72)).astype(np.float32)
    G = dev(g0).clone()
    ws = torch.empty(16 * 40 * 72, device=DEV)
    ddZ, dX = dev(dZ), dev(X)
    hip.gemm(40, 72, rows, ddZ.data_ptr(), 40, 1, dX.data_ptr(), 72, 1, G.data_ptr(), 72, accumulate=True, split_k=16,
             workspace=ws.data_ptr())
    ref = g0 + dZ.astype(np.float64).T @ X.astype(np.float64)
    assert rel_close(G.cpu().numpy(), ref, 1e-5, scale=float(np.sqrt(rows)))


@pytest.mark.parametrize("rows,H,A", [(16384, 512, 6), (16384, 512, 1), (3000, 64, 9), (777, 128, 16), (100, 32, 3),
                                      (5000, 516, 7)])
def test_gemm_narrow_heads(rows, H, A):
    """The three products of a Linear(H, A <= 16) head (forward, weight + bias gradient, data gradient) take the
    bandwidth kernels of csrc/skinny.h; same contract as the MFMA path."""
    rng = np.random.default_rng(rows + H + A)
    X = np.maximum(rng.standard_normal((rows, H)), 0).astype(np.float32)
    W = (rng.standard_normal((A, H)) / np.sqrt(H)).astype(np.float32)
    b = rng.standard_normal(A).astype(np.float32)
    dZ = rng.standard_normal((rows, A)).astype(np.float32)
    dX_, dW_, db_, ddZ = dev(X), dev(W), dev(b), dev(dZ)
    # forward: Y = X W^T + b, then accumulated a second time without bias (the LSTM-style accumulate contract)
    Y = torch.full((rows, A), np.nan, device=DEV)
    hip.gemm(rows, A, H, dX_.data_ptr(), H, 0, dW_.data_ptr(), H, 0, Y.data_ptr(), A, bias=db_.data_ptr())
    ref = X.astype(np.float64) @ W.astype(np.float64).T + b
    assert rel_close(Y.cpu().numpy(), ref, 1e-5, scale=float(np.sqrt(H)))
    hip.gemm(rows, A, H, dX_.data_ptr(), H, 0, dW_.data_ptr(), H, 0, Y.data_ptr(), A, accumulate=True)
    assert rel_close(Y.cpu().numpy(), 2 * ref - b, 1e-5, scale=float(np.sqrt(H)))
    # weight gradient (+ bias gradient from the same pass), accumulating
    g0, s0 = rng.standard_normal((A, H)).astype(np.float32), rng.standard_normal(A).astype(np.float32)
    G, S = dev(g0).clone(), dev(s0).clone()
    ws = torch.empty(8 * A * H, device=DEV)
    assert hip.gemm_colsum_ok(A, H, rows, ddZ.data_ptr(), A, dX_.data_ptr(), H, 1) == (rows >= 256 or A % 4 == 0)
    cs = S.data_ptr() if hip.gemm_colsum_ok(A, H, rows, ddZ.data_ptr(), A, dX_.data_ptr(), H, 1) else None
    hip.gemm(A, H, rows, ddZ.data_ptr(), A, 1, dX_.data_ptr(), H, 1, G.data_ptr(), H, accumulate=True, split_k=8,
             workspace=ws.data_ptr(), a_colsum=cs)
    assert rel_close(G.cpu().numpy(), g0 + dZ.astype(np.float64).T @ X.astype(np.float64), 1e-5, scale=float(np.sqrt(rows)))
    if cs is not None:
        assert rel_close(S.cpu().numpy(), s0 + dZ.astype(np.float64).sum(0), 1e-5, scale=float(np.sqrt(rows)))
    # data gradient with the producer's ReLU mask, plain and accumulated
    D = torch.full((rows, H), np.nan, device=DEV)
    hip.gemm(rows, H, A, ddZ.data_ptr(), A, 0, dW_.data_ptr(), H, 1, D.data_ptr(), H, dact_src=dX_.data_ptr(), ld_dact=H,
             dact=1)
    refd = (dZ.astype(np.float64) @ W.astype(np.float64)) * (X > 0)
    assert rel_close(D.cpu().numpy(), refd, 1e-5, scale=1.0)
    hip.gemm(rows, H, A, ddZ.data_ptr(), A, 0, dW_.data_ptr(), H, 1, D.data_ptr(), H, accumulate=True)
    assert rel_close(D.cpu().numpy(), refd + dZ.astype(np.float64) @ W.astype(np.float64), 1e-5, scale=1.0)


def test_gemm_strided_views():
    """Operands / outputs that are column slices of wider buffers (observation concat, head slices)."""
    rng = np.random.default_rng(9)
    M, N, K, LD = 200, 24, 40, 100
    wide = rng.standard_normal((M, LD)).astype(np.float32)
    W = rng.standard_normal((N, K)).astype(np.float32)
    dwide, dW = dev(wide), dev(W)
    out = torch.zeros((M, 64), device=DEV)
    hip.gemm(M, N, K, dwide.data_ptr() + 4 * 12, LD, 0, dW.data_ptr(), K, 0, out.data_ptr() + 4 * 8, 64)
    ref = wide[:, 12:12 + K].astype(np.float64) @ W.astype(np.float64).T
    got = out.cpu().numpy()
    assert rel_close(got[:, 8:8 + N], ref, 1e-5, scale=float(np.sqrt(K)))
    assert (got[:, :8] == 0).all() and (got[:, 8 + N:] == 0).all()


# ------------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("rows,D", [(1, 4), (1000, 4), (777, 64), (300, 512), (65, 100), (5000, 16), (3333, 32), (4099, 128),
                                    (257, 20), (1031, 96), (90000, 64), (513, 66), (37, 1024), (37, 1408), (3000, 2816),
                                    (5, 11264), (16384, 512), (1000, 256), (777, 768)])
def test_layernorm_fwd_bwd(rows, D):
    rng = np.random.default_rng(rows + D)
    x = (rng.standard_normal((rows, D)) * 2 + 0.5).astype(np.float32)
    x = np.maximum(x, 0)  # pretend it came out of a ReLU, to exercise the fused mask
    gamma = (1 + 0.1 * rng.standard_normal(D)).astype(np.float32)
    beta = (0.1 * rng.standard_normal(D)).astype(np.float32)
    dy = rng.standard_normal((rows, D)).astype(np.float32)
    dx_, dg_, db_ = dev(x), dev(gamma), dev(beta)
    y = torch.empty((rows, D), device=DEV)
    mean = torch.empty(rows, device=DEV)
    rstd = torch.empty(rows, device=DEV)
    hip.layernorm_fwd(dx_.data_ptr(), D, dg_.data_ptr(), db_.data_ptr(), rows, D, y.data_ptr(), D, mean.data_ptr(),
                      rstd.data_ptr())
    tx = torch.from_numpy(x).double().requires_grad_(True)
    tg = torch.from_numpy(gamma).double().requires_grad_(True)
    tb = torch.from_numpy(beta).double().requires_grad_(True)
    pre = tx.clone()
    ty = torch.nn.functional.layer_norm(torch.relu(pre), (D,), tg, tb, 1e-5)
    assert rel_close(y.cpu().numpy(), ty.detach().numpy(), 1e-5, scale=1.0)
    ty.backward(torch.from_numpy(dy).double())
    ddy = dev(dy)
    dxo = torch.empty((rows, D), device=DEV)
    dgo = torch.zeros(D, device=DEV)
    dbo = torch.zeros(D, device=DEV)
    amax = torch.zeros(1, device=DEV)  # the data gradient's range from the same pass (whichever kernel takes the shape)
    hip.layernorm_bwd(ddy.data_ptr(), D, dx_.data_ptr(), D, dg_.data_ptr(), mean.data_ptr(), rstd.data_ptr(), rows, D,
                      dxo.data_ptr(), D, 1, dgo.data_ptr(), dbo.data_ptr(), dx_absmax=amax.data_ptr())
    assert float(amax) == float(dxo.abs().max())
    assert rel_close(dxo.cpu().numpy(), tx.grad.numpy(), 2e-5, scale=1.0)
    assert rel_close(dgo.cpu().numpy(), tg.grad.numpy(), 2e-5, scale=float(np.sqrt(rows)))
    assert rel_close(dbo.cpu().numpy(), tb.grad.numpy(), 2e-5, scale=float(np.sqrt(rows)))


# ------------------------------------------------------------------------------------------------ convolution pieces
def test_obs_ln_im2col_and_affine_bwd():
    rng = np.random.default_rng(3)
    n, C, H, W, k, s = 5, 4, 84, 84, 8, 4
    obs = rng.integers(0, 256, (n, C, H, W), dtype=np.uint8)
    gamma = (1 + 0.1 * rng.standard_normal((C, H, W))).astype(np.float32)
    beta = (0.1 * rng.standard_normal((C, H, W))).astype(np.float32)
    dobs, dg, db = dev(obs), dev(gamma), dev(beta)
    mean = torch.empty(n, device=DEV)
    rstd = torch.empty(n, device=DEV)
    hip.obs_ln_stats(dobs.data_ptr(), True, n, C * H * W, mean.data_ptr(), rstd.data_ptr())
    x64 = obs.astype(np.float64)
    mu = x64.reshape(n, -1).mean(1)
    var = x64.reshape(n, -1).var(1)
    assert rel_close(mean.cpu().numpy(), mu, 1e-6) and rel_close(rstd.cpu().numpy(), 1 / np.sqrt(var + 1e-5), 1e-6)
    OH = (H - k) // s + 1
    P = torch.empty((n * OH * OH, C * k * k), device=DEV)
    hip.im2col_obs_ln(dobs.data_ptr(), True, mean.data_ptr(), rstd.data_ptr(), dg.data_ptr(), db.data_ptr(), n, C, H, W, k,
                      k, s, P.data_ptr())
    xn = torch.nn.functional.layer_norm(torch.from_numpy(x64), (C, H, W), torch.from_numpy(gamma).double(),
                                        torch.from_numpy(beta).double(), 1e-5)
    ref = torch.nn.functional.unfold(xn, k, stride=s).transpose(1, 2).reshape(n * OH * OH, C * k * k)
    assert rel_close(P.cpu().numpy(), ref.numpy(), 1e-5, scale=1.0)
    # float32 observations take the same path
    dobs_f = dev(obs.astype(np.float32))
    hip.obs_ln_stats(dobs_f.data_ptr(), False, n, C * H * W, mean.data_ptr(), rstd.data_ptr())
    assert rel_close(mean.cpu().numpy(), mu, 1e-6)
    # affine gradients: d/dgamma, d/dbeta of sum(P * dP)
    dP = rng.standard_normal((n * OH * OH, C * k * k)).astype(np.float32)
    tg = torch.from_numpy(gamma).double().requires_grad_(True)
    tb = torch.from_numpy(beta).double().requires_grad_(True)
    xn2 = torch.nn.functional.layer_norm(torch.from_numpy(x64), (C, H, W), tg, tb, 1e-5)
    p2 = torch.nn.functional.unfold(xn2, k, stride=s).transpose(1, 2).reshape(n * OH * OH, C * k * k)
    (p2 * torch.from_numpy(dP).double()).sum().backward()
    gg = torch.zeros((C, H, W), device=DEV)
    gb = torch.zeros((C, H, W), device=DEV)
    hip.obs_ln_stats(dobs.data_ptr(), True, n, C * H * W, mean.data_ptr(), rstd.data_ptr())
    ddP = dev(dP)
    hip.obs_ln_affine_bwd(ddP.data_ptr(), dobs.data_ptr(), True, mean.data_ptr(), rstd.data_ptr(), n, C, H, W, k, k, s,
                          gg.data_ptr(), gb.data_ptr())
    assert rel_close(gg.cpu().numpy(), tg.grad.numpy(), 2e-5, scale=1.0)
    assert rel_close(gb.cpu().numpy(), tb.grad.numpy(), 2e-5, scale=1.0)


@pytest.mark.parametrize("H,C,k,s", [(20, 32, 4, 2), (9, 64, 3, 1), (11, 8, 5, 3)])
def test_im2col_col2im_nhwc(H, C, k, s):
    rng = np.random.default_rng(H)
    n = 6
    x = rng.standard_normal((n, H, H, C)).astype(np.float32)
    OH = (H - k) // s + 1
    P = torch.empty((n * OH * OH, k * k * C), device=DEV)
    dx_ = dev(x)
    hip.im2col_ndhwc(dx_.data_ptr(), n, (1, H, H, C), (1, k, k), s, P.data_ptr())
    xt = torch.from_numpy(x).permute(0, 3, 1, 2).double().requires_grad_(True)  # NCHW for unfold
    u = torch.nn.functional.unfold(xt, k, stride=s)  # [n, C*k*k, L] with (c,kh,kw) order
    u = u.reshape(n, C, k, k, OH * OH).permute(0, 4, 2, 3, 1).reshape(n * OH * OH, k * k * C)  # -> (kh,kw,c)
    assert np.array_equal(P.cpu().numpy(), u.detach().numpy().astype(np.float32))
    dP = rng.standard_normal((n * OH * OH, k * k * C)).astype(np.float32)
    (u * torch.from_numpy(dP).double()).sum().backward()
    ymask = rng.standard_normal((n, H, H, C)).astype(np.float32)
    dX = torch.empty((n, H, H, C), device=DEV)
    ddP, dym = dev(dP), dev(ymask)  # keep the device copies alive across the asynchronous launch
    hip.col2im_ndhwc(ddP.data_ptr(), n, (1, H, H, C), (1, k, k), s, dym.data_ptr(), 1, dX.data_ptr())
    torch.cuda.synchronize()
    ref = xt.grad.permute(0, 2, 3, 1).numpy() * (ymask > 0)
    assert rel_close(dX.cpu().numpy(), ref, 1e-5, scale=1.0)


@pytest.mark.parametrize("M,N,K,split", [(64, 512, 5000, 1), (512, 3136, 16384, 4), (8, 512, 777, 1), (132, 68, 1001, 3),
                                         (32, 36, 40000, 8), (4, 4, 3, 1)])
def test_gemm_a_colsum(M, N, K, split):
    """Weight-gradient shape C[M,N] += A^T B with A [K,M], B [K,N] both k-major; a_colsum[M] += sum_k A[k, :]."""
    rng = np.random.default_rng(M + N + K)
    A = rng.standard_normal((K, M)).astype(np.float32)
    B = rng.standard_normal((K, N)).astype(np.float32)
    c0 = rng.standard_normal((M, N)).astype(np.float32)
    s0 = rng.standard_normal(M).astype(np.float32)
    dA, dB, dC, dS = dev(A), dev(B), dev(c0).clone(), dev(s0).clone()
    ws = torch.empty(max(split * M * N, 1), device=DEV)
    assert hip.gemm_colsum_ok(M, N, K, dA.data_ptr(), M, dB.data_ptr(), N, 1)
    hip.gemm(M, N, K, dA.data_ptr(), M, 1, dB.data_ptr(), N, 1, dC.data_ptr(), N, accumulate=True, split_k=split,
             workspace=ws.data_ptr(), a_colsum=dS.data_ptr())
    assert rel_close(dC.cpu().numpy(), c0 + A.astype(np.float64).T @ B.astype(np.float64), 1e-5, scale=float(np.sqrt(K)))
    assert rel_close(dS.cpu().numpy(), s0 + A.astype(np.float64).sum(0), 1e-5, scale=float(np.sqrt(K)))
    # operands the float4 path cannot stage are refused loudly (the caller then runs srl_colsum)
    if M <= 16:  # narrow products take the bandwidth kernels, which have no alignment demands on A
        return
    assert not hip.gemm_colsum_ok(M + 1, N, K, dA.data_ptr(), M + 1, dB.data_ptr(), N, 1)
    with pytest.raises(hip.HipError):
        hip.gemm(M, N, K, dA.data_ptr() + 4, M, 1, dB.data_ptr(), N, 1, dC.data_ptr(), N, accumulate=True,
                 a_colsum=dS.data_ptr())


def test_colsum_copy2d():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((10000, 70)).astype(np.float32)
    out = torch.ones(70, device=DEV)
    dxx = dev(x)
    hip.colsum(dxx.data_ptr(), 70, 10000, 70, out.data_ptr(), accumulate=True)
    assert rel_close(out.cpu().numpy(), 1 + x.astype(np.float64).sum(0), 1e-5, scale=100.0)
    dst = torch.zeros((100, 50), device=DEV)
    src = dev(x[:100])
    hip.copy2d(src.data_ptr(), 70, dst.data_ptr() + 4 * 5, 50, 100, 30)
    assert np.array_equal(dst.cpu().numpy()[:, 5:35], x[:100, :30])


# ------------------------------------------------------------------------------------------------ optimiser
@pytest.mark.parametrize("max_norm", [None, 0.5, 1e9])
def test_adam_matches_torch(max_norm):
    rng = np.random.default_rng(4)
    n = 100003
    p0 = rng.standard_normal(n).astype(np.float32)
    tp = torch.from_numpy(p0.copy()).requires_grad_(True)
    opt = torch.optim.Adam([tp], lr=3e-4)
    p, m, v = dev(p0).clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    sumsq = torch.zeros(1, dtype=torch.float64, device=DEV)
    gn = torch.zeros(1, device=DEV)
    for step in range(1, 4):
        g = rng.standard_normal(n).astype(np.float32) * 0.01
        tp.grad = torch.from_numpy(g.copy())
        ref_norm = torch.nn.utils.clip_grad_norm_([tp], max_norm if max_norm is not None else 1e30)
        opt.step()
        dg = dev(g)
        hip.grad_sumsq(dg, sumsq)
        hip.adam_step(p, dg, m, v, 3e-4, 0.9, 0.999, 1e-8, 0.0, False, step, max_norm=-1 if max_norm is None else max_norm,
                      sumsq=sumsq, grad_norm_out=gn)
        assert abs(gn.item() - ref_norm.item()) <= 1e-5 * ref_norm.item()
        assert rel_close(p.cpu().numpy(), tp.detach().numpy(), 1e-6, scale=1.0), step


# ------------------------------------------------------------------------------------------------ implicit-GEMM convolutions
def _signbits(a):
    """Sign-bit mask of a tensor the way the kernels keep it: bit e & 31 of word e >> 5 = (element e > 0)."""
    flat = np.ascontiguousarray(a).reshape(-1) > 0
    flat = np.concatenate([flat, np.zeros((-flat.size) % 32, bool)])
    return np.packbits(flat, bitorder="little").view(np.uint32)


def _conv_ref(x_nhwc, w_ohwi, bias, stride, act):
    """float64 reference on the CPU: NHWC in/out, weights [Cout, KH, KW, Cin]."""
    xt = torch.from_numpy(x_nhwc).double().permute(0, 3, 1, 2).requires_grad_(True)
    wt = torch.from_numpy(w_ohwi).double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    bt = torch.from_numpy(bias).double().requires_grad_(True)
    z = torch.nn.functional.conv2d(xt, wt, bt, stride=stride)
    y = torch.relu(z) if act == 1 else z
    return xt, wt, bt, y


@pytest.mark.parametrize("n,H,Cin,k,s,Cout", [(6, 20, 32, 4, 2, 64), (5, 9, 64, 3, 1, 64), (7, 11, 8, 5, 3, 12),
                                              (300, 9, 64, 3, 1, 64), (3, 12, 4, 3, 2, 132),
                                              # enough images for the data gradient's position-grouped tiles (border
                                              # taps skipped), image counts that do not fill the last group
                                              (1100, 9, 64, 3, 1, 64), (600, 20, 32, 4, 2, 64), (1030, 7, 8, 3, 1, 16),
                                              (1024, 6, 16, 5, 1, 32)])
def test_conv2d_nhwc_implicit(n, H, Cin, k, s, Cout):
    rng = np.random.default_rng(n + H)
    x = np.maximum(rng.standard_normal((n, H, H, Cin)), 0).astype(np.float32)  # a post-ReLU activation
    w = (rng.standard_normal((Cout, k, k, Cin)) / np.sqrt(k * k * Cin)).astype(np.float32)
    b = rng.standard_normal(Cout).astype(np.float32)
    d = hip.conv_desc(n, H, H, Cin, k, k, s, Cout, act=1)
    assert hip.conv2d_supported(d, False)
    OH = (H - k) // s + 1
    dx_, dw_, db_ = dev(x), dev(w), dev(b)
    y = torch.full((n, OH, OH, Cout), np.nan, device=DEV)
    hip.conv2d_nhwc_fwd(d, dx_.data_ptr(), dw_.data_ptr(), db_.data_ptr(), y.data_ptr())
    xt, wt, bt, yref = _conv_ref(x, w, b, s, 1)
    assert rel_close(y.cpu().numpy(), yref.permute(0, 2, 3, 1).detach().numpy(), 1e-5, scale=1.0)
    if Cout % 32 == 0:  # the same launch also leaves the sign bits of y: exactly (y > 0), and y itself unchanged
        ym = torch.full((n * OH * OH * Cout // 32,), -1, dtype=torch.int32, device=DEV)
        y_m = torch.full_like(y, np.nan)
        hip.conv2d_nhwc_fwd(d, dx_.data_ptr(), dw_.data_ptr(), db_.data_ptr(), y_m.data_ptr(), y_mask=ym.data_ptr())
        assert torch.equal(y_m, y)
        assert np.array_equal(ym.cpu().numpy().view(np.uint32), _signbits(y.cpu().numpy()))
    # backward: dz = upstream gradient w.r.t. the pre-activation
    dz = (rng.standard_normal((n, OH, OH, Cout)) * (yref.permute(0, 2, 3, 1).detach().numpy() > 0)).astype(np.float32)
    z = torch.nn.functional.conv2d(xt, wt, bt, stride=s)
    z.backward(torch.from_numpy(dz).double().permute(0, 3, 1, 2))
    ddz = dev(dz)
    g0 = rng.standard_normal(w.shape).astype(np.float32)
    gw = dev(g0).clone()
    ws = torch.empty(max(hip.conv2d_wgrad_workspace(d), 1), device=DEV)
    gb0 = rng.standard_normal(Cout).astype(np.float32)
    gb = dev(gb0).clone()  # the bias gradient comes out of the same kernel (column sums of dz), accumulating
    hip.conv2d_nhwc_wgrad(d, dx_.data_ptr(), ddz.data_ptr(), gw.data_ptr(), ws.data_ptr(), gb.data_ptr())
    ref_gw = g0 + wt.grad.permute(0, 2, 3, 1).numpy()
    assert rel_close(gw.cpu().numpy(), ref_gw, 1e-5, scale=float(np.sqrt(n * OH * OH)))
    assert rel_close(gb.cpu().numpy(), gb0 + bt.grad.numpy(), 1e-5, scale=float(np.sqrt(n * OH * OH)))
    wtp = torch.empty(hip.conv2d_dgrad_weight_elems(d), device=DEV)
    hip.conv2d_dgrad_repack(d, dw_.data_ptr(), wtp.data_ptr())
    dxo = torch.full((n, H, H, Cin), np.nan, device=DEV)
    hip.conv2d_nhwc_dgrad(d, ddz.data_ptr(), wtp.data_ptr(), dx_.data_ptr(), 1, dxo.data_ptr())
    ref_dx = xt.grad.permute(0, 2, 3, 1).numpy() * (x > 0)
    assert rel_close(dxo.cpu().numpy(), ref_dx, 1e-5, scale=1.0)
    # the ReLU derivative from the sign bits of x instead of its floats: the same gradient, bit for bit
    if Cin % 32 == 0:
        xm = dev(_signbits(x).view(np.int32))
        dxm = torch.full((n, H, H, Cin), np.nan, device=DEV)
        hip.conv2d_nhwc_dgrad(d, ddz.data_ptr(), wtp.data_ptr(), None, 1, dxm.data_ptr(), x_mask=xm.data_ptr())
        assert torch.equal(dxm, dxo)
    torch.cuda.synchronize()


@pytest.mark.parametrize("n,C,H,k,s,Cout,u8", [(5, 4, 84, 8, 4, 32, True), (3, 2, 20, 4, 4, 8, False),
                                               (130, 4, 84, 8, 4, 32, True)])
def test_conv2d_obs_implicit(n, C, H, k, s, Cout, u8):
    rng = np.random.default_rng(n)
    obs = rng.integers(0, 256, (n, C, H, H), dtype=np.uint8)
    if not u8:
        obs = obs.astype(np.float32) / 7
    gamma = (1 + 0.1 * rng.standard_normal((C, H, H))).astype(np.float32)
    beta = (0.1 * rng.standard_normal((C, H, H))).astype(np.float32)
    w = (rng.standard_normal((Cout, C, k, k)) / np.sqrt(C * k * k)).astype(np.float32)
    b = rng.standard_normal(Cout).astype(np.float32)
    d = hip.conv_desc(n, H, H, C, k, k, s, Cout, act=1)
    assert hip.conv2d_supported(d, True)
    OH = (H - k) // s + 1
    dobs, dg, dbt, dw_, db_ = dev(obs), dev(gamma), dev(beta), dev(w), dev(b)
    mean = torch.empty(n, device=DEV)
    rstd = torch.empty(n, device=DEV)
    hip.obs_ln_stats(dobs.data_ptr(), u8, n, C * H * H, mean.data_ptr(), rstd.data_ptr())
    y = torch.full((n, OH, OH, Cout), np.nan, device=DEV)
    hip.conv2d_obs_fwd(d, dobs.data_ptr(), u8, mean.data_ptr(), rstd.data_ptr(), dg.data_ptr(), dbt.data_ptr(),
                       dw_.data_ptr(), db_.data_ptr(), y.data_ptr())
    tg = torch.from_numpy(gamma).double().requires_grad_(True)
    tb = torch.from_numpy(beta).double().requires_grad_(True)
    tw = torch.from_numpy(w).double().requires_grad_(True)
    tbias = torch.from_numpy(b).double().requires_grad_(True)
    xn = torch.nn.functional.layer_norm(torch.from_numpy(obs.astype(np.float64)), (C, H, H), tg, tb, 1e-5)
    z = torch.nn.functional.conv2d(xn, tw, tbias, stride=s)
    yref = torch.relu(z)
    assert rel_close(y.cpu().numpy(), yref.permute(0, 2, 3, 1).detach().numpy(), 1e-5, scale=1.0)
    dz = (rng.standard_normal((n, OH, OH, Cout)) * (yref.permute(0, 2, 3, 1).detach().numpy() > 0)).astype(np.float32)
    z.backward(torch.from_numpy(dz).double().permute(0, 3, 1, 2))
    ddz = dev(dz)
    outs = [torch.zeros(s_, device=DEV) for s_ in (w.shape, (Cout,), gamma.shape, beta.shape)]
    ws = torch.empty(hip.conv2d_obs_bwd_workspace(d), device=DEV)
    hip.conv2d_obs_bwd(d, dobs.data_ptr(), u8, mean.data_ptr(), rstd.data_ptr(), dg.data_ptr(), dbt.data_ptr(),
                       dw_.data_ptr(), ddz.data_ptr(), *[o.data_ptr() for o in outs], ws.data_ptr())
    sc = float(np.sqrt(n * OH * OH))
    for got, ref, name in zip(outs, (tw.grad, tbias.grad, tg.grad, tb.grad), ("dw", "db", "dgamma", "dbeta")):
        assert rel_close(got.cpu().numpy(), ref.numpy(), 2e-5, scale=sc if name in ("dw", "db") else float(np.sqrt(n))), name
    torch.cuda.synchronize()


def _frames(rng, n, C, H, kind):
    """uint8 frame stacks: uniform noise, or Atari-like (a flat background with a few objects: small variance around a
    large mean -- what stresses the bf16 path's mean correction, obs_bf16.h), or nearly black."""
    if kind == "noise":
        return rng.integers(0, 256, (n, C, H, H), dtype=np.uint8)
    bg = 87 if kind == "pong" else 0
    obs = np.full((n, C, H, H), bg, dtype=np.uint8)
    for i in range(n):
        for _ in range(6):
            y, x, hh, ww = rng.integers(0, H - 8), rng.integers(0, H - 8), rng.integers(1, 8), rng.integers(1, 8)
            obs[i, :, y:y + hh, x:x + ww] = rng.integers(100, 256)
    return obs


@pytest.mark.parametrize("n,u8,kind", [(5, True, "noise"), (70, True, "noise"), (3, False, "noise"), (200, True, "pong"),
                                       (1100, True, "noise"), (96, True, "black")])
def test_conv2d_obs_space_to_depth_path(n, u8, kind):
    """Strided first layer on the space-to-depth'd observation == the planar convolution (Atari geometry).  uint8 frames
    with n >= 32 take the bf16 matrix-core kernels (obs_bf16.h: bytes x three exact bf16 planes); the others the float32
    MFMA kernels.  Both against float64 torch."""
    from srl_amd.algorithm.netspec import ParamInfo
    rng = np.random.default_rng(n)
    C, H, k, s, Cout = 4, 84, 8, 4, 32
    obs = _frames(rng, n, C, H, kind)
    if not u8:
        obs = obs.astype(np.float32) / 3
    gamma = (1 + 0.1 * rng.standard_normal((C, H, H))).astype(np.float32)
    beta = (0.1 * rng.standard_normal((C, H, H))).astype(np.float32)
    w = (rng.standard_normal((Cout, C, k, k)) / np.sqrt(C * k * k)).astype(np.float32)
    b = rng.standard_normal(Cout).astype(np.float32)
    pw = ParamInfo("w", w.shape, layout="conv_s2d", s2d=s)
    pg = ParamInfo("g", gamma.shape, layout="ln_s2d", s2d=s)
    t = torch.from_numpy
    dobs = dev(obs)
    dg, dbt = pg.to_internal(t(gamma)).to(DEV), pg.to_internal(t(beta)).to(DEV)
    dw_, db_ = pw.to_internal(t(w)).to(DEV), dev(b)
    s2d = torch.empty_like(dobs)
    mean, rstd = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
    hip.obs_space_to_depth(dobs.data_ptr(), u8, n, C, H, H, s, s2d.data_ptr(), mean.data_ptr(), rstd.data_ptr())
    ref_s2d = obs.reshape(n, C, H // s, s, H // s, s).transpose(0, 2, 4, 1, 3, 5).reshape(n, -1)
    assert np.array_equal(s2d.cpu().numpy().reshape(n, -1), ref_s2d)
    x64 = obs.astype(np.float64).reshape(n, -1)
    assert rel_close(mean.cpu().numpy(), x64.mean(1), 1e-6) and rel_close(rstd.cpu().numpy(), 1 / np.sqrt(x64.var(1) + 1e-5), 1e-6)
    Hb, Cb, kb = H // s, C * s * s, k // s
    d = hip.conv_desc(n, Hb, Hb, Cb, kb, kb, 1, Cout, act=1)
    assert hip.conv2d_supported(d, 2)
    OH = (H - k) // s + 1
    y = torch.full((n, OH, OH, Cout), np.nan, device=DEV)
    hip.conv2d_obs_fwd(d, s2d.data_ptr(), u8, mean.data_ptr(), rstd.data_ptr(), dg.data_ptr(), dbt.data_ptr(),
                       dw_.data_ptr(), db_.data_ptr(), y.data_ptr(), channels_last=True)
    tg, tb = t(gamma).double().requires_grad_(True), t(beta).double().requires_grad_(True)
    tw, tbias = t(w).double().requires_grad_(True), t(b).double().requires_grad_(True)
    xn = torch.nn.functional.layer_norm(t(obs.astype(np.float64)), (C, H, H), tg, tb, 1e-5)
    z = torch.nn.functional.conv2d(xn, tw, tbias, stride=s)
    yref = torch.relu(z)
    assert rel_close(y.cpu().numpy(), yref.permute(0, 2, 3, 1).detach().numpy(), 1e-5, scale=1.0)
    # position-batched form (affine folded into per-position weights); needs >= 64 samples to be selected
    fws = torch.empty(hip.conv2d_obs_fwd_workspace(d), device=DEV)
    y2 = torch.full((n, OH, OH, Cout), np.nan, device=DEV)
    hip.conv2d_obs_fwd(d, s2d.data_ptr(), u8, mean.data_ptr(), rstd.data_ptr(), dg.data_ptr(), dbt.data_ptr(),
                       dw_.data_ptr(), db_.data_ptr(), y2.data_ptr(), channels_last=True, ws_ptr=fws.data_ptr())
    assert rel_close(y2.cpu().numpy(), yref.permute(0, 2, 3, 1).detach().numpy(), 1e-5, scale=1.0)
    for wsp, yy in ((None, y), (fws.data_ptr(), y2)):  # sign bits of the ReLU output from the same launches
        ym = torch.full((n * OH * OH * Cout // 32,), -1, dtype=torch.int32, device=DEV)
        y_m = torch.full_like(y, np.nan)
        hip.conv2d_obs_fwd(d, s2d.data_ptr(), u8, mean.data_ptr(), rstd.data_ptr(), dg.data_ptr(), dbt.data_ptr(),
                           dw_.data_ptr(), db_.data_ptr(), y_m.data_ptr(), channels_last=True, ws_ptr=wsp, y_mask=ym.data_ptr())
        assert torch.equal(y_m, yy)
        assert np.array_equal(ym.cpu().numpy().view(np.uint32), _signbits(yy.cpu().numpy()))
    dz = (rng.standard_normal((n, OH, OH, Cout)) * (yref.permute(0, 2, 3, 1).detach().numpy() > 0)).astype(np.float32)
    z.backward(t(dz).double().permute(0, 3, 1, 2))
    ddz = dev(dz)
    outs = [torch.zeros(w.size, device=DEV), torch.zeros(Cout, device=DEV), torch.zeros(gamma.size, device=DEV),
            torch.zeros(beta.size, device=DEV)]
    ws = torch.empty(hip.conv2d_obs_bwd_workspace(d), device=DEV)
    hip.conv2d_obs_bwd(d, s2d.data_ptr(), u8, mean.data_ptr(), rstd.data_ptr(), dg.data_ptr(), dbt.data_ptr(),
                       dw_.data_ptr(), ddz.data_ptr(), *[o.data_ptr() for o in outs], ws.data_ptr(), channels_last=True)
    got = [pw.to_reference(outs[0].cpu()), outs[1].cpu(), pg.to_reference(outs[2].cpu()), pg.to_reference(outs[3].cpu())]
    sc = float(np.sqrt(n * OH * OH))
    for g_, ref, name in zip(got, (tw.grad, tbias.grad, tg.grad, tb.grad), ("dw", "db", "dgamma", "dbeta")):
        assert rel_close(g_.numpy(), ref.numpy(), 2e-5, scale=sc if name in ("dw", "db") else float(np.sqrt(n))), name
    torch.cuda.synchronize()
    if u8 and n >= 32:  # the two first-layer implementations against each other: same bytes, same weights
        import os
        os.environ["SRL_OBS_BF16"] = "0"
        try:
            y3 = torch.full((n, OH, OH, Cout), np.nan, device=DEV)
            hip.conv2d_obs_fwd(d, s2d.data_ptr(), u8, mean.data_ptr(), rstd.data_ptr(), dg.data_ptr(), dbt.data_ptr(),
                               dw_.data_ptr(), db_.data_ptr(), y3.data_ptr(), channels_last=True, ws_ptr=fws.data_ptr())
            outs3 = [torch.zeros_like(o) for o in outs]
            hip.conv2d_obs_bwd(d, s2d.data_ptr(), u8, mean.data_ptr(), rstd.data_ptr(), dg.data_ptr(), dbt.data_ptr(),
                               dw_.data_ptr(), ddz.data_ptr(), *[o.data_ptr() for o in outs3], ws.data_ptr(), channels_last=True)
            torch.cuda.synchronize()
        finally:
            del os.environ["SRL_OBS_BF16"]
        ref64 = yref.permute(0, 2, 3, 1).detach().numpy()
        e_bf16, e_f32 = np.abs(y2.cpu().numpy() - ref64).max(), np.abs(y3.cpu().numpy() - ref64).max()
        assert e_bf16 <= max(4 * e_f32, 2e-6), (e_bf16, e_f32)  # no worse than the float32 MFMA chain, up to noise
        for a_, b_, name in zip(outs, outs3, ("dw", "db", "dgamma", "dbeta")):
            assert rel_close(a_.cpu().numpy(), b_.cpu().numpy(), 2e-5, scale=sc if name in ("dw", "db") else float(np.sqrt(n))), name


# ------------------------------------------------------------------------------------------------ encoder pieces, any rank
@pytest.mark.parametrize("M,N,K,akm,bkm,split", [(16384 + 64, 3136, 512, 0, 1, 1), (4096, 1100, 2048, 0, 0, 1),
                                                 (512, 3136, 16384, 1, 1, 5), (64, 576, 40000, 1, 1, 21)])
def test_gemm_tile_numbering_large(M, N, K, akm, bkm, split):
    """Shapes that take the L2-aware tile numberings of the bf16x3 kernel (column groups when B exceeds the L2, k-ranges of
    a split-K product folded into the one-dimensional grid): the numbering must not change which tile computes what."""
    g = torch.Generator(device="cpu").manual_seed(M + N)
    A = torch.randn((K, M) if akm else (M, K), generator=g).to(DEV)
    B = torch.randn((K, N) if bkm else (N, K), generator=g).to(DEV)
    C = torch.full((M, N), float("nan"), device=DEV)
    ws = torch.empty(split * M * N, device=DEV) if split > 1 else None
    hip.gemm(M, N, K, A.data_ptr(), A.shape[1], akm, B.data_ptr(), B.shape[1], bkm, C.data_ptr(), N, split_k=split,
             workspace=None if ws is None else ws.data_ptr())
    ref = (A.double().T if akm else A.double()) @ (B.double() if bkm else B.double().T)
    err = (C.double() - ref).abs().max().item()
    assert err <= 1e-5 * float(np.sqrt(K)) * 4, err


@pytest.mark.parametrize("vol,pads", [((1, 1, 37, 3), (0, 0, 2)), ((1, 9, 7, 8), (0, 1, 1)), ((5, 4, 6, 2), (1, 2, 0)),
                                      ((3, 4, 5, 2), (2, 3, 4))])
@pytest.mark.parametrize("mode", ["zeros", "reflect", "replicate", "circular"])
def test_pad_crop_ndhwc(vol, pads, mode):
    """Borders per nn.ConvNd's padding_mode against torch.nn.functional.pad, and the adjoint against its autograd."""
    rng = np.random.default_rng(sum(vol))
    n = 3
    D, H, W, C = vol
    x = rng.standard_normal((n, D, H, W, C)).astype(np.float32)
    pv = tuple(d + 2 * p for d, p in zip(vol[:3], pads))
    xt = torch.from_numpy(x).permute(0, 4, 1, 2, 3).double().requires_grad_(True)  # [n, C, D, H, W]
    tpad = (pads[2], pads[2], pads[1], pads[1], pads[0], pads[0])
    yt = torch.nn.functional.pad(xt, tpad, mode="constant" if mode == "zeros" else mode)
    y = torch.full((n, *pv, C), float("nan"), device=DEV)
    dx_ = dev(x)
    hip.pad_ndhwc(dx_.data_ptr(), n, vol, pads, y.data_ptr(), hip.PAD_MODES[mode])
    assert np.array_equal(y.cpu().numpy(), yt.permute(0, 2, 3, 4, 1).detach().numpy().astype(np.float32))
    if mode == "zeros":
        back = torch.full((n, D, H, W, C), float("nan"), device=DEV)
        hip.crop_ndhwc(y.data_ptr(), n, vol, pads, back.data_ptr(), hip.PAD_MODES[mode])
        assert np.array_equal(back.cpu().numpy().view(np.uint32), x.view(np.uint32)), "crop(pad(x)) == x, bit for bit"
    dy = rng.standard_normal((n, *pv, C)).astype(np.float32)
    (yt * torch.from_numpy(dy).permute(0, 4, 1, 2, 3).double()).sum().backward()
    back = torch.full((n, D, H, W, C), float("nan"), device=DEV)
    ddy = dev(dy)
    hip.crop_ndhwc(ddy.data_ptr(), n, vol, pads, back.data_ptr(), hip.PAD_MODES[mode])
    assert rel_close(back.cpu().numpy(), xt.grad.permute(0, 2, 3, 4, 1).numpy(), 1e-6, scale=1.0)


@pytest.mark.parametrize("vol,win", [((1, 1, 59, 3), (1, 1, 2)), ((1, 23, 19, 4), (1, 2, 2)), ((9, 8, 7, 2), (2, 2, 2))])
@pytest.mark.parametrize("dact", [0, 1, 2])
def test_maxpool_ndhwc_matches_torch(vol, win, dact):
    """MaxPool{1,2,3}d(2) and its backward (first maximum of a window, torch's rule) times the activation derivative; ties
    are made frequent by quantising the input."""
    rng = np.random.default_rng(sum(vol) + dact)
    n = 4
    D, H, W, C = vol
    x = np.round(rng.standard_normal((n, D, H, W, C)) * 2).astype(np.float32) / 2
    if dact == 1:
        x = np.maximum(x, 0)
    elif dact == 2:
        x = np.tanh(x).astype(np.float32)
    nd = sum(w == 2 for w in win)
    xt = torch.from_numpy(x).permute(0, 4, 1, 2, 3).double().requires_grad_(True)  # [n, C, D, H, W]
    pool = {1: torch.nn.functional.max_pool1d, 2: torch.nn.functional.max_pool2d, 3: torch.nn.functional.max_pool3d}[nd]
    yt = pool(xt.reshape(n, C, *vol[3 - nd:3]), 2)
    out_sp = tuple(d // w for d, w in zip(vol[:3], win))
    y = torch.full((n, *out_sp, C), float("nan"), device=DEV)
    dx_ = dev(x)
    hip.maxpool_ndhwc_fwd(dx_.data_ptr(), n, vol, win, y.data_ptr())
    yref = yt.reshape(n, C, *out_sp).permute(0, 2, 3, 4, 1).detach().numpy()
    assert np.array_equal(y.cpu().numpy(), yref.astype(np.float32))
    dy = rng.standard_normal((n, *out_sp, C)).astype(np.float32)
    (yt.reshape(n, C, *out_sp) * torch.from_numpy(dy).permute(0, 4, 1, 2, 3).double()).sum().backward()
    g = xt.grad.permute(0, 2, 3, 4, 1).numpy()
    dref = g * {0: 1.0, 1: (x > 0), 2: 1.0 - x.astype(np.float64)**2}[dact]
    dxo = torch.full((n, D, H, W, C), float("nan"), device=DEV)
    ddy = dev(dy)
    hip.maxpool_ndhwc_bwd(ddy.data_ptr(), dx_.data_ptr(), n, vol, win, dact, dxo.data_ptr())
    assert rel_close(dxo.cpu().numpy(), dref, 1e-6, scale=1.0)


@pytest.mark.parametrize("vol,kern,s", [((1, 1, 40, 3), (1, 1, 5), 2), ((1, 9, 9, 4), (1, 3, 3), 1), ((6, 7, 5, 2), (2, 3, 2), 1),
                                        ((7, 7, 7, 3), (3, 3, 3), 2), ((3, 5, 4, 8), (2, 3, 2), 1)])
def test_im2col_col2im_ndhwc(vol, kern, s):
    """The patch matrix reproduces torch's convolution of the matching rank through one GEMM, and col2im is its adjoint."""
    rng = np.random.default_rng(sum(vol) + s)
    n, Co = 3, 5
    D, H, W, C = vol
    KD, KH, KW = kern
    x = rng.standard_normal((n, D, H, W, C)).astype(np.float32)
    w = rng.standard_normal((Co, C, KD, KH, KW)).astype(np.float32)
    out_sp = tuple((d - k) // s + 1 for d, k in zip(vol[:3], kern))
    m, kdim = n * int(np.prod(out_sp)), KD * KH * KW * C
    P = torch.full((m, kdim), float("nan"), device=DEV)
    dx_ = dev(x)
    hip.im2col_ndhwc(dx_.data_ptr(), n, vol, kern, s, P.data_ptr())
    xt = torch.from_numpy(x).permute(0, 4, 1, 2, 3).double().requires_grad_(True)
    yt = torch.nn.functional.conv3d(xt, torch.from_numpy(w).double(), stride=s)  # [n, Co, OD, OH, OW]
    wmat = torch.from_numpy(w).permute(0, 2, 3, 4, 1).reshape(Co, kdim).double()  # [Cout][KD][KH][KW][Cin]
    y = (P.cpu().double() @ wmat.T).reshape(n, *out_sp, Co).permute(0, 4, 1, 2, 3)
    assert torch.allclose(y, yt.detach(), rtol=1e-6, atol=1e-6)
    dy = rng.standard_normal(tuple(yt.shape)).astype(np.float32)
    (yt * torch.from_numpy(dy).double()).sum().backward()
    dP = (torch.from_numpy(dy).permute(0, 2, 3, 4, 1).reshape(m, Co).double() @ wmat).float().to(DEV)
    ymask = rng.standard_normal((n, D, H, W, C)).astype(np.float32)
    dym = dev(ymask)
    dX = torch.full((n, D, H, W, C), float("nan"), device=DEV)
    hip.col2im_ndhwc(dP.data_ptr(), n, vol, kern, s, dym.data_ptr(), 1, dX.data_ptr())
    ref = xt.grad.permute(0, 2, 3, 4, 1).numpy() * (ymask > 0)
    assert rel_close(dX.cpu().numpy(), ref, 2e-5, scale=1.0)


@pytest.mark.parametrize("u8", [True, False])
def test_obs_ln_nhwc_fwd_bwd(u8):
    """Whole-observation LayerNorm written out channels-last (the general encoder path) against torch's layer_norm."""
    rng = np.random.default_rng(5 + u8)
    n, C, H, W = 6, 3, 7, 5
    obs = rng.integers(0, 256, (n, C, H, W)).astype(np.uint8) if u8 else rng.standard_normal((n, C, H, W)).astype(np.float32)
    gamma = rng.standard_normal((C, H, W)).astype(np.float32)
    beta = rng.standard_normal((C, H, W)).astype(np.float32)
    xt = torch.from_numpy(obs.astype(np.float64))
    tg, tb = torch.from_numpy(gamma).double().requires_grad_(True), torch.from_numpy(beta).double().requires_grad_(True)
    yt = torch.nn.functional.layer_norm(xt, (C, H, W), tg, tb, 1e-5)
    dobs, dg, db_ = dev(obs), dev(gamma), dev(beta)
    mean, rstd = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
    hip.obs_ln_stats(dobs.data_ptr(), u8, n, C * H * W, mean.data_ptr(), rstd.data_ptr())
    y = torch.full((n, H, W, C), float("nan"), device=DEV)
    hip.obs_ln_nhwc(dobs.data_ptr(), u8, mean.data_ptr(), rstd.data_ptr(), dg.data_ptr(), db_.data_ptr(), n, C, H, W, y.data_ptr())
    assert rel_close(y.cpu().numpy(), yt.permute(0, 2, 3, 1).detach().numpy(), 1e-5, scale=1.0)
    dy = rng.standard_normal((n, H, W, C)).astype(np.float32)
    (yt.permute(0, 2, 3, 1) * torch.from_numpy(dy).double()).sum().backward()
    gg, gb = torch.zeros((C, H, W), device=DEV), torch.zeros((C, H, W), device=DEV)
    ddy = dev(dy)
    hip.obs_ln_nhwc_bwd(ddy.data_ptr(), dobs.data_ptr(), u8, mean.data_ptr(), rstd.data_ptr(), n, C, H, W, gg.data_ptr(),
                        gb.data_ptr())
    assert rel_close(gg.cpu().numpy(), tg.grad.numpy(), 2e-5, scale=1.0)
    assert rel_close(gb.cpu().numpy(), tb.grad.numpy(), 2e-5, scale=1.0)


@pytest.mark.parametrize("M,N,K", [(300, 64, 128), (1000, 3136, 512), (130, 96, 72)])
def test_gemm_sign_masks(M, N, K):
    """srl_gemm_desc.mask_out / dact_mask: the forward product leaves the sign bits of its ReLU output; a data gradient reads
    them instead of the floats and returns the same matrix bit for bit."""
    rng = np.random.default_rng(M + N)
    a, w, b = (rng.standard_normal(sh).astype(np.float32) for sh in ((M, K), (N, K), (N,)))
    da, dw_, db_ = dev(a), dev(w), dev(b)
    y = torch.full((M, N), np.nan, device=DEV)
    hip.gemm(M, N, K, da.data_ptr(), K, 0, dw_.data_ptr(), K, 0, y.data_ptr(), N, bias=db_.data_ptr(), act=1)
    if N % 32 == 0:
        y2 = torch.full_like(y, np.nan)
        ym = torch.full((M * N // 32,), -1, dtype=torch.int32, device=DEV)
        hip.gemm(M, N, K, da.data_ptr(), K, 0, dw_.data_ptr(), K, 0, y2.data_ptr(), N, bias=db_.data_ptr(), act=1,
                 mask_out=ym.data_ptr())
        assert torch.equal(y2, y)
        assert np.array_equal(ym.cpu().numpy().view(np.uint32), _signbits(y.cpu().numpy()))
    # dX = dZ W' masked by the derivative of the ReLU that produced X's layer input x_in [M, N]: floats vs bits
    x_in = np.maximum(rng.standard_normal((M, N)), 0).astype(np.float32)
    dz = rng.standard_normal((M, K)).astype(np.float32)
    w2 = rng.standard_normal((K, N)).astype(np.float32)  # [out = K, in = N]: B(k, j) k-major
    ddz, dw2, dxin = dev(dz), dev(w2), dev(x_in)
    g_f = torch.full((M, N), np.nan, device=DEV)
    hip.gemm(M, N, K, ddz.data_ptr(), K, 0, dw2.data_ptr(), N, 1, g_f.data_ptr(), N, dact_src=dxin.data_ptr(), ld_dact=N, dact=1)
    if N % 32:
        return
    g_m = torch.full((M, N), np.nan, device=DEV)
    xm = dev(_signbits(x_in).view(np.int32))
    hip.gemm(M, N, K, ddz.data_ptr(), K, 0, dw2.data_ptr(), N, 1, g_m.data_ptr(), N, ld_dact=N, dact=1, dact_mask=xm.data_ptr())
    assert torch.equal(g_m, g_f)
    ref = (dz.astype(np.float64) @ w2.astype(np.float64)) * (x_in > 0)
    assert rel_close(g_m.cpu().numpy(), ref, 1e-5, scale=float(np.sqrt(K)))


def test_conv2d_runs_of_images(monkeypatch):
    """A batch is walked in runs of images (csrc/conv.hip images_per_launch; SRL_CONV_RUN_IMAGES forces short runs here): forward
    with mask and range, data gradient from the mask, weight gradient, and the first layer through a slot index -- equal to the
    single-run call (bit for bit where no sum runs over the images)."""
    rng = np.random.default_rng(5)
    n, H, Cin, k, s, Cout = 1000, 20, 32, 4, 2, 64
    x = np.maximum(rng.standard_normal((n, H, H, Cin)), 0).astype(np.float32)
    w = (rng.standard_normal((Cout, k, k, Cin)) / np.sqrt(k * k * Cin)).astype(np.float32)
    b = rng.standard_normal(Cout).astype(np.float32)
    d = hip.conv_desc(n, H, H, Cin, k, k, s, Cout, act=1)
    OH = (H - k) // s + 1
    dx_, dw_, db_ = dev(x), dev(w), dev(b)
    dz = dev((rng.standard_normal((n, OH, OH, Cout))).astype(np.float32))
    wtp = torch.empty(hip.conv2d_dgrad_weight_elems(d), device=DEV)
    hip.conv2d_dgrad_repack(d, dw_.data_ptr(), wtp.data_ptr())
    xm = dev(_signbits(x).view(np.int32))
    ws = torch.empty(max(hip.conv2d_wgrad_workspace(d), 1), device=DEV)

    def run_all():
        y = torch.full((n, OH, OH, Cout), np.nan, device=DEV)
        ym = torch.full((n * OH * OH * Cout // 32,), -1, dtype=torch.int32, device=DEV)
        yr = torch.zeros(1, device=DEV)
        hip.conv2d_nhwc_fwd(d, dx_.data_ptr(), dw_.data_ptr(), db_.data_ptr(), y.data_ptr(), y_absmax=yr.data_ptr(),
                            y_mask=ym.data_ptr())
        gx = torch.full((n, H, H, Cin), np.nan, device=DEV)
        hip.conv2d_nhwc_dgrad(d, dz.data_ptr(), wtp.data_ptr(), None, 1, gx.data_ptr(), x_mask=xm.data_ptr())
        gw, gb = torch.zeros((Cout, k, k, Cin), device=DEV), torch.zeros(Cout, device=DEV)
        hip.conv2d_nhwc_wgrad(d, dx_.data_ptr(), dz.data_ptr(), gw.data_ptr(), ws.data_ptr(), gb.data_ptr())
        torch.cuda.synchronize()
        return y, ym, yr, gx, gw, gb

    # the first layer on ring rows: frames of 1400 slots, the batch's 1000 rows through a slot index
    slots = 1400
    frames = torch.from_numpy(rng.integers(0, 256, (slots, 21, 21, 64), dtype=np.uint8)).to(DEV)
    fmean = frames.reshape(slots, -1).float().mean(1)
    frstd = 1.0 / torch.sqrt(frames.reshape(slots, -1).float().var(1, unbiased=False) + 1e-5)
    ridx = torch.from_numpy(rng.permutation(slots)[:n].astype(np.int32)).to(DEV)
    d1 = hip.conv_desc(n, 21, 21, 64, 2, 2, 1, 32, act=1)
    assert hip.conv2d_obs_row_index_supported(d1, True, True)
    g1 = dev((1 + 0.1 * rng.standard_normal(21 * 21 * 64)).astype(np.float32))
    b1 = dev((0.1 * rng.standard_normal(21 * 21 * 64)).astype(np.float32))
    w1 = dev((rng.standard_normal(32 * 256) / 16).astype(np.float32))
    wb1 = dev(rng.standard_normal(32).astype(np.float32))
    dz1 = dev(rng.standard_normal((n, 20, 20, 32)).astype(np.float32))
    fws = torch.empty(hip.conv2d_obs_fwd_workspace(d1), device=DEV)
    bws = torch.empty(hip.conv2d_obs_bwd_workspace(d1), device=DEV)

    def run_first():
        y1 = torch.full((n, 20, 20, 32), np.nan, device=DEV)
        m1 = torch.full((n * 400,), -1, dtype=torch.int32, device=DEV)
        hip.conv2d_obs_fwd(d1, frames.data_ptr(), True, fmean.data_ptr(), frstd.data_ptr(), g1.data_ptr(), b1.data_ptr(),
                           w1.data_ptr(), wb1.data_ptr(), y1.data_ptr(), channels_last=True, ws_ptr=fws.data_ptr(),
                           row_index=ridx, y_mask=m1.data_ptr())
        outs = [torch.zeros(32 * 256, device=DEV), torch.zeros(32, device=DEV), torch.zeros(21 * 21 * 64, device=DEV),
                torch.zeros(21 * 21 * 64, device=DEV)]
        hip.conv2d_obs_bwd(d1, frames.data_ptr(), True, fmean.data_ptr(), frstd.data_ptr(), g1.data_ptr(), b1.data_ptr(),
                           w1.data_ptr(), dz1.data_ptr(), *[o.data_ptr() for o in outs], bws.data_ptr(), channels_last=True,
                           row_index=ridx)
        torch.cuda.synchronize()
        return y1, m1, outs

    one = run_all()
    first = run_first()
    monkeypatch.setenv("SRL_CONV_RUN_IMAGES", "300")  # 1000 images in 4 equal runs of 250
    runs = run_all()
    first_runs = run_first()
    for a, b_, name in zip(one[:4], runs[:4], ("y", "mask", "range", "dx")):
        assert torch.equal(a, b_), name
    for a, b_, name in zip(one[4:], runs[4:], ("dw", "db")):
        assert rel_close(b_.cpu().numpy(), a.cpu().numpy(), 1e-5, scale=float(a.abs().max())), name
    assert torch.equal(first[0], first_runs[0]) and torch.equal(first[1], first_runs[1])
    for a, b_, name in zip(first[2], first_runs[2], ("dw1", "db1", "dgamma", "dbeta")):
        assert rel_close(b_.cpu().numpy(), a.cpu().numpy(), 2e-5, scale=float(a.abs().max())), name


@pytest.mark.timeout(600)
def test_conv2d_more_than_2_gib():
    """Activation tensors beyond 32-bit byte offsets (2.2 GB of input, 43 000 images of 20x20x32): the forward pass and the data
    gradient of the far end of the batch equal the same images presented alone."""
    n, H, Cin, k, s, Cout = 43000, 20, 32, 4, 2, 64
    g = torch.Generator(device=DEV).manual_seed(3)
    x = torch.relu(torch.randn((n, H, H, Cin), device=DEV, generator=g))
    assert x.numel() * 4 > 2 ** 31
    w = torch.randn((Cout, k, k, Cin), device=DEV, generator=g) * 0.05
    b = torch.randn(Cout, device=DEV, generator=g)
    OH = (H - k) // s + 1
    d = hip.conv_desc(n, H, H, Cin, k, k, s, Cout, act=1)
    y = torch.full((n, OH, OH, Cout), float("nan"), device=DEV)
    hip.conv2d_nhwc_fwd(d, x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr())
    tail = 700  # the last images lie beyond 2^31 bytes in x
    dt = hip.conv_desc(tail, H, H, Cin, k, k, s, Cout, act=1)
    xt = x[n - tail:].contiguous()
    yt = torch.empty((tail, OH, OH, Cout), device=DEV)
    hip.conv2d_nhwc_fwd(dt, xt.data_ptr(), w.data_ptr(), b.data_ptr(), yt.data_ptr())
    assert torch.equal(y[n - tail:], yt) and not torch.isnan(y).any()
    dz = torch.randn((n, OH, OH, Cout), device=DEV, generator=g)
    wtp = torch.empty(hip.conv2d_dgrad_weight_elems(d), device=DEV)
    hip.conv2d_dgrad_repack(d, w.data_ptr(), wtp.data_ptr())
    gx = torch.full((n, H, H, Cin), float("nan"), device=DEV)
    hip.conv2d_nhwc_dgrad(d, dz.data_ptr(), wtp.data_ptr(), x.data_ptr(), 1, gx.data_ptr())
    gxt = torch.empty((tail, H, H, Cin), device=DEV)
    hip.conv2d_nhwc_dgrad(dt, dz[n - tail:].contiguous().data_ptr(), wtp.data_ptr(), xt.data_ptr(), 1, gxt.data_ptr())
    assert torch.equal(gx[n - tail:], gxt) and not torch.isnan(gx).any()
    # dense product with a 2.4 GB operand: the far rows against torch
    del gx, dz, y
    M, K, N = 300000, 2048, 64
    a = torch.randn((M, K), device=DEV, generator=g)
    assert a.numel() * 4 > 2 ** 31
    wd = torch.randn((N, K), device=DEV, generator=g) * 0.02
    out = torch.full((M, N), float("nan"), device=DEV)
    hip.gemm(M, N, K, a.data_ptr(), K, 0, wd.data_ptr(), K, 0, out.data_ptr(), N)
    ref = a[M - 512:].double() @ wd.double().t()
    assert rel_close(out[M - 512:].cpu().numpy(), ref.cpu().numpy(), 1e-5, scale=float(ref.detach().abs().max()))
    assert not torch.isnan(out).any()


@pytest.mark.parametrize("M,N,K,akm,bkm,split,extra", [
    (256, 64, 64, 0, 0, 1, "bias"), (256, 64, 4 * 3, 0, 0, 1, "bias"), (100, 64, 64, 0, 1, 1, "acc"),
    (64, 64, 256, 1, 1, 4, "colsum"), (64, 64, 100, 1, 1, 1, "colsum"), (64, 8, 32, 1, 1, 1, "colsum"),
    (8, 64, 12, 1, 1, 1, "colsum"), (1000, 8, 64, 1, 1, 1, "colsum"), (40, 128, 512, 1, 0, 2, "acc")])
def test_gemm_small_products(M, N, K, akm, bkm, split, extra):
    """Products of at most 65 536 outputs and K <= 512 (the layers of the CartPole-sized configurations) take 64 x 64 tiles
    with 64-deep k-steps (gemm.hip): every orientation, a K shorter than one step, fused column sums of a single-step product
    (whose first tile must not be counted twice), split-K -- against float64."""
    rng = np.random.default_rng(M + N + K)
    A = dev(rng.standard_normal((K, M) if akm else (M, K)).astype(np.float32))
    B = dev(rng.standard_normal((K, N) if bkm else (N, K)).astype(np.float32))
    C0 = dev(rng.standard_normal((M, N)).astype(np.float32))
    C = C0.clone()
    bias = dev(rng.standard_normal(N).astype(np.float32))
    cs0 = dev(rng.standard_normal(M).astype(np.float32))
    cs = cs0.clone()
    ws = torch.empty(split * M * N, device=DEV) if split > 1 else None
    hip.dispatch_counts(reset=True)
    hip.gemm(M, N, K, A.data_ptr(), A.shape[1], akm, B.data_ptr(), B.shape[1], bkm, C.data_ptr(), N, split_k=split,
             workspace=None if ws is None else ws.data_ptr(), accumulate=extra in ("acc", "colsum"),
             bias=bias.data_ptr() if extra == "bias" else None, act=1 if extra == "bias" else 0,
             a_colsum=cs.data_ptr() if extra == "colsum" else None)
    import os
    if os.environ.get("SRL_SMALL_GEMM", "1")[:1] != "0":  # (the A/B switch sends them back to the general kernels)
        assert hip.dispatch_counts()["gemm3"] == 1
    Ad = A.double().T if akm else A.double()
    ref = Ad @ (B.double() if bkm else B.double().T)
    ref = torch.relu(ref + bias.double()) if extra == "bias" else ref + C0.double()
    assert rel_close(C.cpu().numpy(), ref.cpu().numpy(), 1e-5, scale=float(np.sqrt(K)))
    if extra == "colsum":
        assert rel_close(cs.cpu().numpy(), (cs0.double() + Ad.sum(1)).cpu().numpy(), 1e-5, scale=float(np.sqrt(K)))


@pytest.mark.parametrize("rows,dims,acts", [(256, (4, 64, 64, 2), (1, 1, 0)), (37, (10, 128, 33, 1), (2, 2, 0)),
                                            (1000, (48, 64, 9), (1, 0)), (5003, (4, 64, 64, 2), (2, 1, 0)),
                                            (65536, (4, 64, 64, 1), (2, 2, 0)), (700, (33, 40, 6), (2, 0))])
def test_mlp_chain_fused(rows, dims, acts):
    """srl_mlp_fwd / srl_mlp_bwd (csrc/mlp_small.hip): LayerNorm -> Linear (+ activation) chains as one launch per direction,
    against float64 autograd: outputs, every parameter gradient, ragged row counts, widths that are not multiples of 16.
    From 512 rows on, chains no wider than 64 run on the float32 matrix cores (csrc/mlp_mfma.h): the cases with 700+ rows.
    (65 536 rows: smooth activations -- among that many rows one has a ReLU pre-activation within float32 rounding of zero, and
    the float64 reference then takes the other branch: both float32 chains agree with each other there to 5e-6.)"""
    rng = np.random.default_rng(rows)
    t = torch
    x = t.from_numpy(rng.standard_normal((rows, dims[0])).astype(np.float32))
    params, layers64 = [], []
    for i in range(len(dims) - 1):  # LayerNorm(d_i) -> Linear(d_i, d_{i+1}) + act
        g = t.from_numpy((1 + 0.1 * rng.standard_normal(dims[i])).astype(np.float32))
        b = t.from_numpy((0.1 * rng.standard_normal(dims[i])).astype(np.float32))
        w = t.from_numpy((rng.standard_normal((dims[i + 1], dims[i])) / np.sqrt(dims[i])).astype(np.float32))
        wb = t.from_numpy((0.1 * rng.standard_normal(dims[i + 1])).astype(np.float32))
        params += [g, b, w, wb]
    dev_p = [p_.to(DEV) for p_ in params]
    dev_g = [t.zeros_like(p_) + 0.5 for p_ in dev_p]  # gradients are accumulated into
    desc = []
    for i in range(len(dims) - 1):
        g, b, w, wb = dev_p[4 * i:4 * i + 4]
        gg, gb, gw, gwb = dev_g[4 * i:4 * i + 4]
        desc.append((0, dims[i], dims[i], 0, g.data_ptr(), b.data_ptr(), gg.data_ptr(), gb.data_ptr()))
        desc.append((1, dims[i], dims[i + 1], acts[i], w.data_ptr(), wb.data_ptr(), gw.data_ptr(), gwb.data_ptr()))
    arr = hip.mlp_layers(desc)
    tld = hip.mlp_tape_floats(arr)
    assert tld == sum(dims[:-1]) + sum(dims[1:-1])
    dx = x.to(DEV)
    tape = t.full((rows, tld), float("nan"), device=DEV)
    y = t.full((rows, dims[-1]), float("nan"), device=DEV)
    hip.mlp_fwd(arr, dx.data_ptr(), dims[0], rows, tape.data_ptr(), tld, y.data_ptr(), dims[-1])
    p64 = [p_.double().requires_grad_(True) for p_ in params]
    h = x.double()
    for i in range(len(dims) - 1):
        g, b, w, wb = p64[4 * i:4 * i + 4]
        h = t.nn.functional.layer_norm(h, (dims[i],), g, b, 1e-5)
        h = h @ w.t() + wb
        h = t.relu(h) if acts[i] == 1 else (t.tanh(h) if acts[i] == 2 else h)
    assert rel_close(y.cpu().numpy(), h.detach().numpy(), 1e-5, scale=1.0)
    dy = t.from_numpy(rng.standard_normal((rows, dims[-1])).astype(np.float32))
    h.backward(dy.double())
    ddy = dy.to(DEV)
    hip.mlp_bwd(arr, dx.data_ptr(), dims[0], rows, tape.data_ptr(), tld, ddy.data_ptr(), dims[-1])
    for got, ref, name in zip(dev_g, p64, [f"{k}{i}" for i in range(len(dims) - 1) for k in ("gamma", "beta", "w", "b")]):
        assert rel_close(got.cpu().numpy() - 0.5, ref.grad.numpy(), 2e-5, scale=float(ref.grad.abs().max()) + 1e-6), name
    assert hip.mlp_bwd_max_rows(arr) >= (1 << 30 if max(dims) <= 64 else 8192)  # the matrix-core chain takes any row count


@needs_f16x2
def test_presplit_weights_give_the_same_bits():
    """srl_presplit + b_presplit / presplit=True: a B operand split once instead of in every tile -- the same pieces, so the
    same results bit for bit: dense forward and data-gradient orientations, the forward convolution, the strided (packed and
    class-by-class) and the stride-1 data gradient (with sign masks); and a product that does not take the two-piece kernel refuses it."""
    rng = np.random.default_rng(11)
    M, N, K = 1000, 512, 3136
    a, w = dev(rng.standard_normal((M, K)).astype(np.float32)), dev((rng.standard_normal((N, K)) * 0.02).astype(np.float32))
    ar, wr = a.abs().max().reshape(1), w.abs().max().reshape(1)
    w2 = torch.empty_like(w)
    hip.presplit(w.data_ptr(), wr.data_ptr(), w2.data_ptr(), w.numel())
    bias = dev(rng.standard_normal(N).astype(np.float32))
    y0, y1 = torch.empty((M, N), device=DEV), torch.full((M, N), np.nan, device=DEV)
    kw = dict(bias=bias.data_ptr(), act=1, a_absmax=ar.data_ptr(), b_absmax=wr.data_ptr())
    assert hip.gemm_two_piece(M, N, K, a.data_ptr(), K, w.data_ptr(), K, ar.data_ptr(), wr.data_ptr())
    hip.gemm(M, N, K, a.data_ptr(), K, 0, w.data_ptr(), K, 0, y0.data_ptr(), N, **kw)
    hip.gemm(M, N, K, a.data_ptr(), K, 0, w2.data_ptr(), K, 0, y1.data_ptr(), N, b_presplit=True, **kw)
    assert torch.equal(y0, y1)
    dz = dev(rng.standard_normal((M, N)).astype(np.float32))
    dzr = dz.abs().max().reshape(1)
    g0, g1 = torch.empty((M, K), device=DEV), torch.full((M, K), np.nan, device=DEV)
    hip.gemm(M, K, N, dz.data_ptr(), N, 0, w.data_ptr(), K, 1, g0.data_ptr(), K, a_absmax=dzr.data_ptr(), b_absmax=wr.data_ptr())
    hip.gemm(M, K, N, dz.data_ptr(), N, 0, w2.data_ptr(), K, 1, g1.data_ptr(), K, a_absmax=dzr.data_ptr(), b_absmax=wr.data_ptr(),
             b_presplit=True)
    assert torch.equal(g0, g1)
    with pytest.raises(hip.HipError, match="b_presplit"):  # no ranges: three bf16 pieces, which cannot take pre-split pieces
        hip.gemm(M, N, K, a.data_ptr(), K, 0, w2.data_ptr(), K, 0, y1.data_ptr(), N, b_presplit=True)
    # (the third: odd H under stride 2 -- the parity classes' row grids differ, so each is a product of its own on its block of wt)
    for (n, H, Cin, k, s_, Cout) in ((600, 20, 32, 4, 2, 64), (600, 9, 64, 3, 1, 64), (600, 21, 64, 4, 2, 64)):
        x = dev(np.maximum(rng.standard_normal((n, H, H, Cin)), 0).astype(np.float32))
        cw = dev((rng.standard_normal((Cout, k, k, Cin)) / np.sqrt(k * k * Cin)).astype(np.float32))
        cb = dev(rng.standard_normal(Cout).astype(np.float32))
        d = hip.conv_desc(n, H, H, Cin, k, k, s_, Cout, act=1)
        OH = (H - k) // s_ + 1
        xr, cwr = x.abs().max().reshape(1), cw.abs().max().reshape(1)
        cw2 = torch.empty_like(cw)
        hip.presplit(cw.data_ptr(), cwr.data_ptr(), cw2.data_ptr(), cw.numel())
        ya, yb = torch.empty((n, OH, OH, Cout), device=DEV), torch.full((n, OH, OH, Cout), np.nan, device=DEV)
        assert hip.conv2d_fwd_two_piece(d, xr.data_ptr(), cwr.data_ptr())
        hip.conv2d_nhwc_fwd(d, x.data_ptr(), cw.data_ptr(), cb.data_ptr(), ya.data_ptr(), x_absmax=xr.data_ptr(), w_absmax=cwr.data_ptr())
        hip.conv2d_nhwc_fwd(d, x.data_ptr(), cw2.data_ptr(), cb.data_ptr(), yb.data_ptr(), x_absmax=xr.data_ptr(), w_absmax=cwr.data_ptr(),
                            presplit=True)
        assert torch.equal(ya, yb)
        cdz = dev(rng.standard_normal((n, OH, OH, Cout)).astype(np.float32))
        cdzr = cdz.abs().max().reshape(1)
        wt = torch.empty(hip.conv2d_dgrad_weight_elems(d), device=DEV)
        hip.conv2d_dgrad_repack(d, cw.data_ptr(), wt.data_ptr())
        wt2 = torch.empty_like(wt)
        hip.presplit(wt.data_ptr(), cwr.data_ptr(), wt2.data_ptr(), wt.numel())
        xm = dev(_signbits(x.cpu().numpy()).view(np.int32))
        da, db_ = torch.empty_like(x), torch.full_like(x, np.nan)
        assert hip.conv2d_dgrad_two_piece(d, cdzr.data_ptr(), cwr.data_ptr())
        hip.conv2d_nhwc_dgrad(d, cdz.data_ptr(), wt.data_ptr(), None, 1, da.data_ptr(), dz_absmax=cdzr.data_ptr(),
                              w_absmax=cwr.data_ptr(), x_mask=xm.data_ptr())
        hip.conv2d_nhwc_dgrad(d, cdz.data_ptr(), wt2.data_ptr(), None, 1, db_.data_ptr(), dz_absmax=cdzr.data_ptr(),
                              w_absmax=cwr.data_ptr(), x_mask=xm.data_ptr(), presplit=True)
        assert torch.equal(da, db_)


# ------------------------------------------------------------------------------------------------ recurrent time loop in one launch
@pytest.mark.parametrize("kind,H,N,C", [("lstm", 64, 100, 7), ("lstm", 32, 33, 3), ("gru", 64, 257, 5), ("gru", 32, 64, 1)])
def test_rnn_time_loop_in_one_launch_matches_the_per_step_path(kind, H, N, C):
    """srl_lstm_seq_fwd/bwd, srl_gru_seq_fwd/bwd (csrc/rnn_seq.hip) against C calls of the per-step entry points with the W_hh
    product between them (csrc/gru.hip, what `HipNet` ran before and still runs for other widths): the same buffers in, the same
    saved values and gradients out (1e-5: the products sum in a different order), ragged row counts, auto-resets inside the chunk."""
    G = 4 if kind == "lstm" else 3
    g = torch.Generator(device=DEV).manual_seed(H + N + C)
    f = lambda *s: torch.randn(*s, device=DEV, generator=g)
    w_hh, b_hh = f(G * H, H) / H ** 0.5, 0.1 * f(G * H)
    pre0 = f(C, N, G * H)                       # W_ih x + b_ih of every step
    h0, c0 = 0.5 * f(N, H), 0.5 * f(N, H)
    reset = (torch.rand(C, N, device=DEV, generator=g) < 0.2).to(torch.uint8)
    dy = f(C, N, H)
    rp = lambda c: reset.data_ptr() + c * N

    def buffers():
        pre, gh = pre0.clone(), torch.zeros(C, N, 3 * H, device=DEV)
        hin, cin = torch.zeros(C, N, H, device=DEV), torch.zeros(C, N, H, device=DEV)
        hip.gru_mask_state(h0.data_ptr(), rp(0), N, H, hin.data_ptr())
        hip.gru_mask_state(c0.data_ptr(), rp(0), N, H, cin.data_ptr())
        return pre, gh, hin, cin, torch.zeros(C, N, H, device=DEV), torch.zeros(C, N, H, device=DEV)

    def run(path):   # the product's time loop (rnnpath), the path named
        pre, gh, hin, cin, y, cnew = buffers()
        k = CELLS[kind]
        s = bufs_of(kind, gi=pre, gh=gh, hin=hin, cin=cin, cnew=cnew, y=y)
        k.fwd(s, w_hh.data_ptr(), b_hh.data_ptr(), rp, N, H, C, path=path)
        fwd = [t.clone() for t in (pre, gh, hin, cin, y, cnew)]
        carry = [torch.zeros(N, H, device=DEV) for _ in range(4)]   # d h_in, d c_in: two alternating sets
        k.bwd(s, dy.data_ptr(), H, w_hh.data_ptr(), rp, N, H, C, lambda c: [t.data_ptr() for t in carry[2 * (c & 1):][:len(k.state)]], path=path)
        return fwd, [pre.clone(), gh.clone()]

    assert hip.rnn_seq_supported(kind, H) and not hip.rnn_seq_supported(kind, 48)
    (f1, b1), (f2, b2) = run("cell"), run("seq")
    names = ("gates", "gh", "hin", "cin", "y", "cnew")
    for name, u, v in zip(names, f1, f2):
        if kind == "gru" and name in ("cin", "cnew"):
            continue
        assert float((u - v).abs().max()) <= 1e-5 * max(1.0, float(u.abs().max())), name
    for name, u, v in zip(("d pre / d gi", "d gh"), b1, b2):
        assert float((u - v).abs().max()) <= 2e-5 * max(1.0, float(u.abs().max())), name


def test_first_layer_position_sums_accumulate_over_calls():
    """srl_conv2d_obs_bwd's `phase`: two calls that share one accumulation (open, then close) add the same four gradients as two
    calls of their own -- the trainer's chunks share one finalisation that way."""
    n = 2048
    g = torch.Generator(device=DEV).manual_seed(5)
    frames = torch.randint(0, 256, (2 * n, 4, 84, 84), dtype=torch.uint8, device=DEV, generator=g)
    s2d, mean, rstd = torch.empty(2 * n, 21, 21, 64, dtype=torch.uint8, device=DEV), torch.empty(2 * n, device=DEV), torch.empty(2 * n, device=DEV)
    hip.obs_space_to_depth(frames.data_ptr(), True, 2 * n, 4, 84, 84, 4, s2d.data_ptr(), mean.data_ptr(), rstd.data_ptr())
    f = lambda *s: torch.randn(*s, device=DEV, generator=g)
    gamma, beta, w = 1 + 0.2 * f(21 * 21 * 64), 0.2 * f(21 * 21 * 64), 0.06 * f(32, 256)
    dz = 1e-3 * f(2 * n, 400, 32)
    desc = hip.conv_desc(n, 21, 21, 64, 2, 2, 1, 32, 1)
    ws = torch.empty(hip.conv2d_obs_bwd_workspace(desc), device=DEV)
    idx = [torch.arange(0, n, device=DEV, dtype=torch.int32), torch.arange(n, 2 * n, device=DEV, dtype=torch.int32)]

    def run(phases):
        outs = [torch.zeros(32 * 256, device=DEV), torch.zeros(32, device=DEV), torch.zeros(21 * 21 * 64, device=DEV), torch.zeros(21 * 21 * 64, device=DEV)]
        for half, ph in enumerate(phases):
            hip.conv2d_obs_bwd(desc, s2d.data_ptr(), True, mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), w.data_ptr(),
                               dz[half * n:(half + 1) * n].data_ptr(), *[o.data_ptr() for o in outs], ws.data_ptr(), channels_last=True,
                               row_index=idx[half], phase=ph)
        return outs
    own, shared = run((3, 3)), run((1, 2))
    for name, u, v in zip(("dw", "db", "dgamma", "dbeta"), own, shared):
        assert float((u - v).abs().max()) <= 2e-6 * float(u.abs().max()), name
    with pytest.raises(hip.HipError):   # only the byte kernels with split slabs accumulate over calls
        small = hip.conv_desc(8, 21, 21, 64, 2, 2, 1, 32, 1)
        hip.conv2d_obs_bwd(small, s2d.data_ptr(), True, mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), w.data_ptr(),
                           dz.data_ptr(), *[o.data_ptr() for o in own], ws.data_ptr(), channels_last=True, phase=1)


_SIG_CHAINS = {
    "c1-actor": [(0, 4, 4, 0), (1, 4, 64, 1), (0, 64, 64, 0), (1, 64, 64, 1), (1, 64, 64, 1), (1, 64, 2, 0)],
    "c1-critic": [(0, 4, 4, 0), (1, 4, 64, 1), (0, 64, 64, 0), (1, 64, 64, 1), (1, 64, 64, 1), (1, 64, 1, 0)],
    "smac-obs": [(0, 30, 30, 0), (1, 30, 64, 1), (0, 64, 64, 0), (1, 64, 64, 1), (0, 64, 64, 0)],
    "smac-state": [(0, 48, 48, 0), (1, 48, 64, 1), (0, 64, 64, 0), (1, 64, 64, 1), (0, 64, 64, 0)],
}


# (the last two: the smallest ragged batches.  The kernels see the rows that the gate filter below keeps, 516 of 534 and 611 of 640:
# from 512 rows on a chain is the matrix-core kernels', and neither count is a multiple of a workgroup's 128 rows.  Of 513 rows
# the filter keeps 488, which is the FMA chain's and needs a tape)
@pytest.mark.parametrize("rows,chain", [(4096, "c1-actor"), (5003, "c1-critic"), (131072, "c1-actor"), (6001, "smac-obs"),
                                        (3001, "smac-state"), (534, "c1-critic"), (640, "smac-obs")])
def test_mlp_chain_shape_kernels_match_the_generic_ones(rows, chain):
    """csrc/mlp_sig.h: the towers of BASELINE configs[0] (LayerNorm 4, 4 -> 64 ReLU, LayerNorm 64, 64 -> 64 ReLU, 64 -> 64 ReLU, 64 ->
    2 | 1) and the encoders of configs[3]'s multi-agent policy (LayerNorm 30 | 48, -> 64 ReLU, LayerNorm, 64 -> 64 ReLU, LayerNorm)
    have kernels instantiated for their shape -- since round 6 on f16 pieces (csrc/mlp_sigh.h: three products per 32 x 32 x 16
    block, 2^-21 per term), with round 5's float32 shape kernels behind SRL_MLP_F16=0.  All three variants (f16 shape kernels,
    float32 shape kernels, the generic matrix-core chain SRL_MLP_SIG=0; a child process each) against float64 autograd, and
    against each other.  Rows in which some ReLU's pre-activation lies within 1e-4 of its layer's range are taken out of the
    batch first: there the derivative is decided by the forward pass's last bits (a float32 pass flips ~1e-7 of the gates of a
    float64 one, the f16 pieces ~1e-6; ONE flipped gate moved a gradient of a 32 768-row batch by 1.4 % of its largest element,
    scripts/mlp_f16_check.py) -- with them in, the comparison measures the data's luck, not the kernels."""
    import subprocess, sys, json
    code = r'''
import sys, json, numpy as np, torch
from srl_amd import hip
rows, chain = int(sys.argv[1]), json.loads(sys.argv[2])
rng = np.random.default_rng(rows)
din, dout = chain[0][1], (chain[-1][2] if chain[-1][0] == 1 else chain[-1][1])
host, dev_p, dev_g, desc = [], [], [], []
for kind, i, o, act in chain:
    if kind == 0:
        w, b = 1 + 0.1 * rng.standard_normal(i), 0.1 * rng.standard_normal(i)
    else:
        w, b = rng.standard_normal((o, i)) / np.sqrt(i), 0.1 * rng.standard_normal(o)
    w, b = torch.from_numpy(w.astype(np.float32)), torch.from_numpy(b.astype(np.float32))
    host += [w, b]
    dw, db = w.cuda(), b.cuda()
    gw, gb = torch.zeros_like(dw), torch.zeros_like(db)
    dev_p += [dw, db]; dev_g += [gw, gb]
    desc.append((kind, i, o, act, dw.data_ptr(), db.data_ptr(), gw.data_ptr(), gb.data_ptr()))
arr = hip.mlp_layers(desc)
assert hip.mlp_tape_floats_at(arr, rows) == 0
x = torch.from_numpy(rng.standard_normal((rows, din)).astype(np.float32))
dy = torch.from_numpy(rng.standard_normal((rows, dout)).astype(np.float32))
with torch.no_grad():   # rows with a gate at rounding distance of zero (float64 forward): out
    hh, keep = x.double(), torch.ones(rows, dtype=torch.bool)
    for li, (kind, i, o, act) in enumerate(chain):
        w, b = host[2 * li].double(), host[2 * li + 1].double()
        hh = torch.nn.functional.layer_norm(hh, (i,), w, b, 1e-5) if kind == 0 else hh @ w.t() + b
        if act == 1:
            keep &= ~(hh.abs() < 1e-4 * hh.abs().max()).any(1)
            hh = torch.relu(hh)
x, dy = x[keep].contiguous(), dy[keep].contiguous()
rows = int(keep.sum())
dx, ddy = x.cuda(), dy.cuda()
y = torch.full((rows, dout), float("nan"), device="cuda")
hip.mlp_fwd(arr, dx.data_ptr(), din, rows, 0, 0, y.data_ptr(), dout)
hip.mlp_bwd(arr, dx.data_ptr(), din, rows, 0, 0, ddy.data_ptr(), dout)
torch.cuda.synchronize()
p64 = [p.double().requires_grad_(True) for p in host]
h = x.double()
for li, (kind, i, o, act) in enumerate(chain):
    w, b = p64[2 * li], p64[2 * li + 1]
    h = torch.nn.functional.layer_norm(h, (i,), w, b, 1e-5) if kind == 0 else h @ w.t() + b
    h = torch.relu(h) if act == 1 else h
h.backward(dy.double())
err_y = float((y.cpu().double() - h.detach()).abs().max())
err_g = max(float((g.cpu().double() - p.grad).abs().max() / (p.grad.abs().max() + 1e-6)) for g, p in zip(dev_g, p64))
np.save(sys.argv[3], np.concatenate([y.cpu().numpy().ravel()] + [g.cpu().numpy().ravel() for g in dev_g]))
print(json.dumps(dict(err_y=err_y, err_g=err_g, n_y=rows * dout, kept=rows)))
'''
    import tempfile
    outs = {}
    with tempfile.TemporaryDirectory() as td:
        for sig in ("1", "f32", "0"):
            env = dict(os.environ, SRL_MLP_SIG="0" if sig == "0" else "1", SRL_MLP_F16="0" if sig == "f32" else "1",
                       PYTHONPATH=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
            r = subprocess.run([sys.executable, "-c", code, str(rows), json.dumps(_SIG_CHAINS[chain]), f"{td}/o{sig}.npy"], env=env,
                               capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stderr[-2000:]
            outs[sig] = (json.loads(r.stdout.strip().splitlines()[-1]), np.load(f"{td}/o{sig}.npy"))
    for sig in ("1", "f32", "0"):
        assert outs[sig][0]["err_y"] < 1e-5 and outs[sig][0]["err_g"] < 2e-5, (sig, outs[sig][0])
    n_y = outs["1"][0]["n_y"]
    assert 0.8 * rows <= outs["1"][0]["kept"] < rows, outs["1"][0]   # (a few per cent of the rows went out)
    ref = outs["0"][1]
    # same fragments, same MFMA order: the float32 shape kernels equal the generic chain to the compiler's choice of fused
    # multiply-adds in the LayerNorm arithmetic; the f16 pieces to 2^-21 per term
    assert np.allclose(outs["f32"][1][:n_y], ref[:n_y], rtol=0, atol=1e-6 * np.abs(ref[:n_y]).max())
    assert np.allclose(outs["1"][1][:n_y], ref[:n_y], rtol=0, atol=4e-6 * np.abs(ref[:n_y]).max())
    for sig in ("1", "f32"):
        assert np.allclose(outs[sig][1][n_y:], ref[n_y:], rtol=0, atol=2e-5 * np.abs(ref[n_y:]).max()), sig


@pytest.mark.parametrize("n,D,heads,in_act", [(1000, 512, (6, 1), 1), (257, 256, (3,), 0), (4099, 512, (7, 1), 2), (64, 1024, (2, 1), 1)])
def test_ln_heads_fused(n, D, heads, in_act):
    """srl_ln_heads_fwd / srl_ln_heads_bwd (csrc/ln_heads.hip): LayerNorm(D) + the heads behind it as one launch per direction,
    against float64 autograd -- head outputs, the stored statistics, dx (times the derivative of the activation that produced x)
    and every parameter gradient (added to what the buffers held); ragged row counts, one and two heads."""
    rng = np.random.default_rng(n + D)
    t = torch
    pre = t.from_numpy(rng.standard_normal((n, D)))
    x64 = t.relu(pre) if in_act == 1 else (t.tanh(pre) if in_act == 2 else pre)
    x64 = x64.float().double()   # the values the kernel sees
    g64 = t.from_numpy(1 + 0.1 * rng.standard_normal(D)).float().double().requires_grad_(True)
    b64 = t.from_numpy(0.1 * rng.standard_normal(D)).float().double().requires_grad_(True)
    W64 = [t.from_numpy(rng.standard_normal((a, D)) / np.sqrt(D)).float().double().requires_grad_(True) for a in heads]
    hb64 = [t.from_numpy(0.1 * rng.standard_normal(a)).float().double().requires_grad_(True) for a in heads]
    assert hip.ln_heads_supported(D, heads)
    xin = x64.clone().requires_grad_(True)
    feat = t.nn.functional.layer_norm(xin, (D,), g64, b64, 1e-5)
    ys = [feat @ W.t() + hb for W, hb in zip(W64, hb64)]
    dys = [t.from_numpy(rng.standard_normal((n, a))).float() for a in heads]
    t.autograd.backward(ys, [d.double() for d in dys])
    x = dev(x64.float().numpy())
    g, b = dev(g64.detach().float().numpy()), dev(b64.detach().float().numpy())
    W, hb = [dev(w.detach().float().numpy()) for w in W64], [dev(v.detach().float().numpy()) for v in hb64]
    y = [t.full((n, a), float("nan"), device=DEV) for a in heads]
    mean, rstd = t.empty(n, device=DEV), t.empty(n, device=DEV)
    hip.ln_heads_fwd(x.data_ptr(), D, n, D, g.data_ptr(), b.data_ptr(), [w.data_ptr() for w in W], [v.data_ptr() for v in hb], list(heads),
                     [o.data_ptr() for o in y], list(heads), mean.data_ptr(), rstd.data_ptr())
    for got, ref in zip(y, ys):
        assert rel_close(got.cpu().numpy(), ref.detach().numpy(), 1e-5, scale=float(ref.detach().abs().max()))
    assert rel_close(mean.cpu().numpy(), x64.mean(1).numpy(), 1e-5, scale=1.0)
    assert rel_close(rstd.cpu().numpy(), (1 / t.sqrt(x64.var(1, unbiased=False) + 1e-5)).numpy(), 1e-5, scale=float(rstd.max()))
    dg, db_ = t.full((D,), 0.5, device=DEV), t.full((D,), 0.5, device=DEV)
    dW, dhb = [t.full((a, D), 0.5, device=DEV) for a in heads], [t.full((a,), 0.5, device=DEV) for a in heads]
    dx = t.full((n, D), float("nan"), device=DEV)
    amax = t.zeros(1, device=DEV)
    ddy = [dev(d.numpy()) for d in dys]
    hip.ln_heads_bwd(x.data_ptr(), D, n, D, g.data_ptr(), b.data_ptr(), mean.data_ptr(), rstd.data_ptr(), [w.data_ptr() for w in W],
                     list(heads), [d.data_ptr() for d in ddy], list(heads), in_act, dx.data_ptr(), D, dg.data_ptr(), db_.data_ptr(),
                     [w.data_ptr() for w in dW], [v.data_ptr() for v in dhb], dx_absmax=amax.data_ptr())
    der = (x64 > 0).double() if in_act == 1 else ((1 - x64 * x64) if in_act == 2 else t.ones_like(x64))
    ref_dx = xin.grad * der
    assert rel_close(dx.cpu().numpy(), ref_dx.numpy(), 2e-5, scale=float(ref_dx.abs().max()))
    assert abs(float(amax) - float(dx.abs().max())) <= 1e-6 * float(dx.abs().max())
    for got, ref, name in [(dg, g64, "dgamma"), (db_, b64, "dbeta")] + [(a_, b_, f"dW{i}") for i, (a_, b_) in enumerate(zip(dW, W64))] + \
            [(a_, b_, f"db{i}") for i, (a_, b_) in enumerate(zip(dhb, hb64))]:
        assert rel_close(got.cpu().numpy() - 0.5, ref.grad.numpy(), 2e-5, scale=float(ref.grad.abs().max()) + 1e-6), name


@pytest.mark.parametrize("rows,chain", [(2000, [(0, 64, 64, 0), (1, 64, 5, 0)]), (4097, [(0, 64, 64, 0), (1, 64, 9, 0)]),
                                        (1024, [(1, 48, 64, 2), (0, 64, 64, 0), (1, 64, 3, 0)])])
def test_mlp_chain_backward_with_input_gradient(rows, chain):
    """srl_mlp_bwd_dx: a fused chain that sits BEHIND other layers (LayerNorm + head after a recurrent cell) also returns d loss /
    d x -- generic matrix-core kernels (5 / 3 outputs) and the kernels instantiated for configs[3]'s tails (9 outputs) -- against
    float64 autograd: dx and every parameter gradient; such a chain keeps no tape."""
    rng = np.random.default_rng(rows)
    t = torch
    din, dout = chain[0][1], chain[-1][2]
    host, dev_g, desc, keep = [], [], [], []
    for kind, i, o, act in chain:
        if kind == 0:
            w, b = 1 + 0.1 * rng.standard_normal(i), 0.1 * rng.standard_normal(i)
        else:
            w, b = rng.standard_normal((o, i)) / np.sqrt(i), 0.1 * rng.standard_normal(o)
        w, b = t.from_numpy(w.astype(np.float32)), t.from_numpy(b.astype(np.float32))
        host += [w, b]
        dw, db_ = w.to(DEV), b.to(DEV)
        gw, gb = t.zeros_like(dw), t.zeros_like(db_)
        keep += [dw, db_]
        dev_g += [gw, gb]
        desc.append((kind, i, o, act, dw.data_ptr(), db_.data_ptr(), gw.data_ptr(), gb.data_ptr()))
    arr = hip.mlp_layers(desc)
    assert hip.mlp_tape_floats_at(arr, rows) == 0
    x = t.from_numpy(rng.standard_normal((rows, din)).astype(np.float32))
    dy = t.from_numpy(rng.standard_normal((rows, dout)).astype(np.float32))
    dx_dev, ddy = x.to(DEV), dy.to(DEV)
    y = t.full((rows, dout), float("nan"), device=DEV)
    dxo = t.full((rows, din), float("nan"), device=DEV)
    hip.mlp_fwd(arr, dx_dev.data_ptr(), din, rows, 0, 0, y.data_ptr(), dout)
    hip.mlp_bwd_dx(arr, dx_dev.data_ptr(), din, rows, ddy.data_ptr(), dout, dxo.data_ptr(), din)
    p64 = [p_.double().requires_grad_(True) for p_ in host]
    x64 = x.double().requires_grad_(True)
    h = x64
    for li, (kind, i, o, act) in enumerate(chain):
        w, b = p64[2 * li], p64[2 * li + 1]
        h = t.nn.functional.layer_norm(h, (i,), w, b, 1e-5) if kind == 0 else h @ w.t() + b
        h = t.relu(h) if act == 1 else (t.tanh(h) if act == 2 else h)
    h.backward(dy.double())
    assert rel_close(y.cpu().numpy(), h.detach().numpy(), 1e-5, scale=float(h.detach().abs().max()))
    assert rel_close(dxo.cpu().numpy(), x64.grad.numpy(), 2e-5, scale=float(x64.grad.abs().max()))
    for k, (g, p_) in enumerate(zip(dev_g, p64)):
        assert rel_close(g.cpu().numpy(), p_.grad.numpy(), 2e-5, scale=float(p_.grad.abs().max()) + 1e-6), k


@pytest.mark.parametrize("chain", [[(0, 64, 64, 0), (1, 64, 9, 0)], [(0, 64, 64, 0), (1, 64, 1, 0)]], ids=["actor-tail", "critic-tail"])
def test_mlp_tails_with_input_gradient_on_every_kernel_family(chain, tmp_path):
    """srl_mlp_fwd / srl_mlp_bwd_dx on configs[3]'s tails (LayerNorm 64, 64 -> 9 | 1) through all three kernel families -- the shape
    kernels on f16 pieces, the shape kernels on float32 MFMAs (SRL_MLP_F16=0) and the generic matrix-core chain (SRL_MLP_SIG=0), a
    child process each -- against float64 autograd: y, dx and every parameter gradient.  513 and 640 rows: just past the row count
    from which the matrix-core kernels take a chain, no multiple of the 128 rows of a workgroup's four tiles (whole tiles past the
    end; at 513 a last tile of one row).  No ReLU in these chains: every row stays in."""
    import subprocess, sys, json
    t = torch
    din, dout = chain[0][1], chain[-1][2]
    cases = {}
    def draw(rows, seed):
        rng = np.random.default_rng(seed)
        host = []
        for kind, i, o, act in chain:
            if kind == 0:
                w, b = 1 + 0.1 * rng.standard_normal(i), 0.1 * rng.standard_normal(i)
            else:
                w, b = rng.standard_normal((o, i)) / np.sqrt(i), 0.1 * rng.standard_normal(o)
            host += [w.astype(np.float32), b.astype(np.float32)]
        return host, rng.standard_normal((rows, din)).astype(np.float32), rng.standard_normal((rows, dout)).astype(np.float32)

    for rows in (513, 640):
        # The head's bias gradient is dy's column sums and LayerNorm's dbeta is W^T times them, and the tolerance is relative to the
        # gradient's own largest element.  The sums of standard normals have standard deviation sqrt(rows), and a draw can cancel far
        # below that (seed 513, one column: 0.17 = 0.007 sqrt(rows)); the f16 pieces' error does not cancel with them: 2^-21 of
        # |w| |dz| per term, ~ 2^-21 sqrt(rows) over the rows.  So: the first seed from `rows` on whose largest column sum reaches
        # half a standard deviation, where the pieces' share is <= 2 * 2^-21 ~ 1e-6 of the gradient -- decided by the data alone.
        seed = rows
        while np.abs(draw(rows, seed)[2].astype(np.float64).sum(0)).max() < 0.5 * np.sqrt(rows):
            seed += 1
        host, x, dy = draw(rows, seed)
        np.savez(tmp_path / f"in{rows}.npz", x=x, dy=dy, **{f"p{k}": p for k, p in enumerate(host)})
        p64 = [t.from_numpy(p).double().requires_grad_(True) for p in host]
        x64 = t.from_numpy(x).double().requires_grad_(True)
        h = x64
        for li, (kind, i, o, act) in enumerate(chain):
            w, b = p64[2 * li], p64[2 * li + 1]
            h = t.nn.functional.layer_norm(h, (i,), w, b, 1e-5) if kind == 0 else h @ w.t() + b
        h.backward(t.from_numpy(dy).double())
        cases[rows] = (h.detach().numpy(), x64.grad.numpy(), [p.grad.numpy() for p in p64])
    code = r'''
import sys, json, numpy as np, torch
from srl_amd import hip
chain, td = json.loads(sys.argv[1]), sys.argv[2]
din, dout = chain[0][1], chain[-1][2]
for rows in (513, 640):
    z = np.load(f"{td}/in{rows}.npz")
    par = [torch.from_numpy(z[f"p{k}"]).cuda() for k in range(2 * len(chain))]
    grads = [torch.zeros_like(p) for p in par]
    desc = [(kind, i, o, act, par[2 * li].data_ptr(), par[2 * li + 1].data_ptr(), grads[2 * li].data_ptr(), grads[2 * li + 1].data_ptr())
            for li, (kind, i, o, act) in enumerate(chain)]
    arr = hip.mlp_layers(desc)
    assert hip.mlp_tape_floats_at(arr, rows) == 0
    x, dy = torch.from_numpy(z["x"]).cuda(), torch.from_numpy(z["dy"]).cuda()
    y = torch.full((rows, dout), float("nan"), device="cuda")
    dx = torch.full((rows, din), float("nan"), device="cuda")
    hip.mlp_fwd(arr, x.data_ptr(), din, rows, 0, 0, y.data_ptr(), dout)
    hip.mlp_bwd_dx(arr, x.data_ptr(), din, rows, dy.data_ptr(), dout, dx.data_ptr(), din)
    torch.cuda.synchronize()
    np.savez(f"{td}/out{rows}_{sys.argv[3]}.npz", y=y.cpu().numpy(), dx=dx.cpu().numpy(), **{f"g{k}": g.cpu().numpy() for k, g in enumerate(grads)})
'''
    for tag, sig, f16 in (("f16", "1", "1"), ("f32", "1", "0"), ("generic", "0", "1")):
        env = dict(os.environ, SRL_MLP_SIG=sig, SRL_MLP_F16=f16, PYTHONPATH=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        r = subprocess.run([sys.executable, "-c", code, json.dumps(chain), str(tmp_path), tag], env=env, capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        for rows, (y64, dx64, g64) in cases.items():
            got = np.load(tmp_path / f"out{rows}_{tag}.npz")
            err = lambda a, b: float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))
            print(tag, rows, "y", err(got["y"], y64), "dx", err(got["dx"], dx64), "grads", [err(got[f"g{k}"], g) for k, g in enumerate(g64)])
            assert rel_close(got["y"], y64, 1e-5, scale=float(np.abs(y64).max())), (tag, rows)
            assert rel_close(got["dx"], dx64, 2e-5, scale=float(np.abs(dx64).max())), (tag, rows)
            for k, g in enumerate(g64):
                assert rel_close(got[f"g{k}"], g, 2e-5, scale=float(np.abs(g).max()) + 1e-6), (tag, rows, k)


@pytest.mark.parametrize("cin,cout,k", [(4, 8, 3), (8, 4, 3), (4, 4, 3), (8, 8, 3), (4, 4, 5), (4, 8, 5)])
@pytest.mark.parametrize("n,H,W", [(3, 7, 9), (5, 36, 70), (64, 20, 35)])
def test_small_channel_direct_convolutions_vs_torch(cin, cout, k, n, H, W):
    """csrc/conv_small.hip (round 6): 3 x 3 and 5 x 5 stride-1 convolutions with 4 / 8 channels as vector-unit kernels -- forward (bias,
    ReLU), data gradient (with the ReLU derivative of the layer's input) and weight / bias gradient (accumulating; slabs per
    wavefront) against float64 torch convolutions: widths that are not multiples of the 32-pixel column blocks, an odd image count
    (the weight gradient pairs images), heights that are not multiples of the three-row window."""
    from srl_amd import hip
    import torch.nn.functional as F
    g = torch.Generator(device="cuda").manual_seed(7 + cin * 10 + cout)
    x = torch.rand(n, H, W, cin, device="cuda", generator=g) * 2 - 1
    x = torch.relu(x)                                      # the input is a ReLU output (its derivative gates dx)
    w = (torch.rand(cout, k, k, cin, device="cuda", generator=g) * 2 - 1) * 0.3
    b = (torch.rand(cout, device="cuda", generator=g) * 2 - 1) * 0.1
    d = hip.conv_desc(n, H, W, cin, k, k, 1, cout, hip.ACT_RELU)
    assert hip.conv2d_small_supported(d)
    y = torch.full((n, H - k + 1, W - k + 1, cout), float("nan"), device="cuda")
    hip.conv2d_small_fwd(d, x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr())
    xr, wr = x.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2)
    ref = torch.relu(F.conv2d(xr, wr, b.double())).permute(0, 2, 3, 1)
    assert float((y.double() - ref).abs().max()) <= 2e-6 * float(ref.abs().max())
    dz = (torch.rand(n, H - k + 1, W - k + 1, cout, device="cuda", generator=g) * 2 - 1) * 1e-2
    dx = torch.full((n, H, W, cin), float("nan"), device="cuda")
    hip.conv2d_small_dgrad(d, dz.data_ptr(), w.data_ptr(), x.data_ptr(), hip.ACT_RELU, dx.data_ptr())
    refd = F.conv_transpose2d(dz.double().permute(0, 3, 1, 2), wr).permute(0, 2, 3, 1) * (x > 0)
    assert float((dx.double() - refd).abs().max()) <= 2e-6 * float(refd.abs().max())
    dx0 = torch.full((n, H, W, cin), float("nan"), device="cuda")
    hip.conv2d_small_dgrad(d, dz.data_ptr(), w.data_ptr(), None, 0, dx0.data_ptr())
    refd0 = F.conv_transpose2d(dz.double().permute(0, 3, 1, 2), wr).permute(0, 2, 3, 1)
    assert float((dx0.double() - refd0).abs().max()) <= 2e-6 * float(refd0.abs().max())
    gw0, gb0 = torch.rand(cout, k, k, cin, device="cuda", generator=g), torch.rand(cout, device="cuda", generator=g)
    gw, gb = gw0.clone(), gb0.clone()
    ws = torch.full((hip.conv2d_small_wgrad_workspace(d),), float("nan"), device="cuda")
    hip.conv2d_small_wgrad(d, x.data_ptr(), dz.data_ptr(), ws.data_ptr(), gw.data_ptr(), gb.data_ptr())
    refw = torch.nn.grad.conv2d_weight(xr, wr.shape, dz.double().permute(0, 3, 1, 2)).permute(0, 2, 3, 1) + gw0.double()
    refb = dz.double().sum((0, 1, 2)) + gb0.double()
    assert float((gw.double() - refw).abs().max()) <= 4e-6 * float(refw.abs().max())
    assert float((gb.double() - refb).abs().max()) <= 4e-6 * float(refb.abs().max())
    gw2, gb2 = gw0.clone(), gb0.clone()
    hip.conv2d_small_wgrad(d, x.data_ptr(), dz.data_ptr(), ws.data_ptr(), gw2.data_ptr(), gb2.data_ptr())
    assert torch.equal(gw, gw2) and torch.equal(gb, gb2)
    assert not hip.conv2d_small_supported(hip.conv_desc(n, H, W, 8, 5, 5, 1, 8)) and not hip.conv2d_small_supported(hip.conv_desc(n, H, W, 4, 3, 3, 2, 4))
    assert not hip.conv2d_small_supported(hip.conv_desc(n, H, W, 16, 3, 3, 1, 4))
