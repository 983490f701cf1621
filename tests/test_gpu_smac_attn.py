"""GPU parity of the agent-specific (attention) SMAC encoders: the fused block against the reference's own modules in float64
(the project's rule, tests/rnn_ref.py::check_vs_float64: an error of at most 3 x the float32 reference's own error plus 2e-6 of the
tensor's largest float64 element), and ``smac_rnn`` + ``mappo`` on nested samples against golden vectors from the real reference
(tests/golden/gen_smac_attn.py)."""
import numpy as np
import pytest
import torch

import srl_amd
from smac_attn_cases import (A, BLOCKS, H, MIXED_POLICY, POLICY, SAMPLE, TRAINER, get64, make_sample, nested, state_dict, unpack)
from srl_amd import hip
from srl_amd.api import config, policy as policy_api, trainer as trainer_api
from srl_amd.namedarray import NamedArray
from srl_amd.runtime import synthetic

srl_amd.register_all()
pytestmark = pytest.mark.gpu

SLOTS = {"obs_self_norm": (hip.EATTN_LN_SELF_W, hip.EATTN_LN_SELF_B), "encoder.embedding.self_embedding.0": (hip.EATTN_SELF_W, hip.EATTN_SELF_B),
         "encoder.attn.pre_norm": (hip.EATTN_PRE_W, hip.EATTN_PRE_B), "encoder.attn.q_linear": (hip.EATTN_Q_W, hip.EATTN_Q_B),
         "encoder.attn.k_linear": (hip.EATTN_K_W, hip.EATTN_K_B), "encoder.attn.v_linear": (hip.EATTN_V_W, hip.EATTN_V_B)}


def close(a, b, rtol, scale=1.0):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool((np.abs(a - b) <= rtol * np.maximum(np.abs(b), scale)).all())


def bound64(ref32, ref64, floor_from=None):
    """The largest error the float64 rule allows a tensor: 3 x the float32 reference's own + 2e-6 of the largest element."""
    top = np.abs(ref64 if floor_from is None else floor_from).max()
    return 3.0 * np.abs(np.asarray(ref32, np.float64) - ref64).max() + 2e-6 * top


def block_case(g, name):
    pre = f"blk_{name}_"
    D, S, n, E = (int(x) for x in g[pre + "dims"])
    keys = [str(k) for k in g[pre + "keys"]]
    dev = "cuda"
    params = {k: torch.from_numpy(v.copy()).to(dev) for k, v in unpack(g, pre + "param").items()}
    grads = {k: torch.zeros_like(v) for k, v in params.items()}
    slots = dict(SLOTS)
    for i, k in enumerate(keys):
        slots[f"{k}_norm"] = (hip.EATTN_LN_KEY_W + i, hip.EATTN_LN_KEY_B + i)
        slots[f"encoder.embedding.{k}_fc.0"] = (hip.EATTN_KEY_W + i, hip.EATTN_KEY_B + i)
    p, gr = {}, {}
    for prefix, (sw, sb) in slots.items():
        for slot, what in ((sw, "weight"), (sb, "bias")):
            p[slot], gr[slot] = params[f"{prefix}.{what}"].data_ptr(), grads[f"{prefix}.{what}"].data_ptr()
    assert len(p) == len(params)
    x = {k: torch.from_numpy(g[pre + "x." + k]).to(dev) for k in ["obs_self"] + keys}
    mask = torch.from_numpy(g[pre + "mask"]).to(dev)
    shapes = [tuple(x[k].shape[1:]) for k in keys]
    desc = hip.entity_attn_desc(D, S, shapes, p, gr)
    leaves = ((x["obs_self"].data_ptr(), S), [(x[k].data_ptr(), c * f) for k, (c, f) in zip(keys, shapes)], (mask.data_ptr(), E))
    return dict(D=D, S=S, n=n, E=E, shapes=shapes, desc=desc, leaves=leaves, grads=grads, keep=(params, x, mask), pre=pre)


@pytest.mark.parametrize("name", BLOCKS)
def test_block_forward_and_backward_vs_float64(name, golden):
    """Every element of the output and of every parameter gradient (no rows, no elements left out).  ``k_linear.bias``: a
    constant added to every key cancels in the softmax, so its true gradient is zero and what the reference holds is rounding
    noise (~1e-16 in float64, ~1e-9 in float32 beside ~1 for ``q_linear.bias``); its floor is taken from ``q_linear.bias``'s
    largest element."""
    g = golden("steps_smac_attn.npz")
    c = block_case(g, name)
    D, n, pre = c["D"], c["n"], c["pre"]
    assert hip.entity_attn_supported(D, c["S"], c["shapes"])
    ldo = 2 * D + 3   # a padded output pitch: the columns behind 2D stay as they are
    out = torch.full((n, ldo), 7.0, dtype=torch.float32, device="cuda")
    hip.entity_attn_fwd(c["desc"], *c["leaves"], n, out.data_ptr(), ldo)
    got = out.cpu().numpy()
    assert (got[:, 2 * D:] == 7.0).all()
    ref32, ref64 = g[pre + "out32"], get64(g, pre + "out", pre + "out32")
    err, bound = np.abs(got[:, :2 * D] - ref64).max(), bound64(ref32, ref64)
    print(f"block {name} out: error {err:.3e} bound {bound:.3e}")
    assert err <= bound
    empty = g[pre + "mask"].sum(1) == 0
    assert (got[empty, D:2 * D] == 0.0).all() and (ref64[empty, D:] == 0.0).all()   # a row without entities pools to exactly 0
    cot = torch.from_numpy(g[pre + "cot"]).to("cuda")
    g32, g64 = unpack(g, pre + "grad"), unpack(g, pre + "grad", f64=True)
    for call in (1, 2):   # the gradients are ADDED: a second call into the same buffers doubles them
        hip.entity_attn_bwd(c["desc"], *c["leaves"], n, cot.data_ptr(), 2 * D)
        for k, t in c["grads"].items():
            floor = g64["encoder.attn.q_linear.bias"] if k == "encoder.attn.k_linear.bias" else None
            err, bound = np.abs(t.cpu().numpy() - call * g64[k]).max(), call * bound64(g32[k], g64[k], floor)
            print(f"block {name} call {call} {k}: error {err:.3e} bound {bound:.3e}")
            assert err <= bound, (k, call, err, bound)


def test_attention_steps_match_reference_golden(golden):
    """Two trainer steps, ``analyze`` and the parameters after each step against the float32 golden at test_gpu_smac.py's
    tolerances."""
    g = golden("steps_smac_attn.npz")
    trainer = trainer_api.make(config.Trainer("mappo", args=TRAINER), config.Policy("smac_rnn", args=POLICY))
    init = state_dict(g, "init")
    for k, v in trainer.policy.get_checkpoint()["state_dict"].items():  # same seed -> the reference's initial weights
        assert np.allclose(v.numpy(), init[k], rtol=1e-4, atol=1e-4), k
    names = [str(s) for s in g["stat_names"]]
    for step in range(2):
        sample, arrays = make_sample(g, step)
        if step == 0:
            Tb = arrays["on_reset"].shape[0]
            ar = trainer.policy.analyze(sample[:Tb - 1], target="ppo")
            lp, ref_lp = ar.new_action_log_probs.cpu().numpy(), g["analyze_new_lp"]
            assert lp.shape == ref_lp.shape == (Tb - 1, 2, A, 1)
            dead = arrays["obs.is_alive"][:Tb - 1] == 0
            assert np.array_equal(np.isneginf(lp), dead) and np.array_equal(np.isneginf(ref_lp), dead)
            assert close(lp[~dead], ref_lp[~dead], 1e-5), "analyze log-probs"
            assert close(ar.state_values.cpu().numpy(), g["analyze_value"], 1e-5), "analyze values"
            assert close(ar.entropy.cpu().numpy(), g["analyze_entropy"], 1e-5), "analyze entropy"
        res = trainer.step(sample)
        ref = dict(zip(names, g[f"step{step}_stats"]))
        for k in ("policy_loss", "value_loss", "entropy", "advantage", "value_targets", "importance_weight", "clip_ratio",
                  "done", "truncated", "grad_norm", "frames", "denorm_value"):
            tol = 1e-5 if k in ("policy_loss", "value_loss", "entropy", "value_targets", "denorm_value") else 1e-4
            print(f"step {step} {k}: {res.stats[k]!r} reference {ref[k]!r}")
            assert abs(res.stats[k] - ref[k]) <= tol * max(abs(ref[k]), 1e-2), (step, k, res.stats[k], ref[k])
        if step == 0:
            assert sample.analyzed_result.adv.shape == g["step0_adv"].shape  # [Tb, B, agents, 1]
            assert close(sample.analyzed_result.adv, g["step0_adv"], 1e-5)
            assert close(sample.analyzed_result.ret, g["step0_ret"], 1e-5)
        sd = trainer.policy.get_checkpoint()["state_dict"]
        want = state_dict(g, f"step{step}")
        assert set(sd) == set(want)
        worst = max((np.abs(sd[k].numpy() - v).max(), k) for k, v in want.items())
        print(f"step {step}: largest parameter difference {worst[0]:.3e} at {worst[1]}")
        for k, v in want.items():
            got = sd[k].numpy()
            assert np.abs(got - v).max() <= 2e-5, (step, k, np.abs(got - v).max())
            if "_RunningMeanStd__" in k:
                assert got.dtype == np.float64 and np.allclose(got, v, rtol=1e-6, atol=1e-13), (step, k)
    assert trainer.policy.version == int(g["version"]) and res.step == trainer.policy.version


def roll_request(g):
    pre = "roll_in."
    tree = nested({k[len(pre):]: g[k] for k in g.files if k.startswith((pre + "local_obs.", pre + "state."))})
    N = g[pre + "on_reset"].shape[0]
    obs = NamedArray(available_action=g[pre + "available_action"], is_alive=np.ones((N, A, 1), np.uint8), **tree)
    return policy_api.RolloutRequest(obs=obs, policy_state=NamedArray(actor_hx=g[pre + "actor_hx"], critic_hx=g[pre + "critic_hx"]),
                                     is_evaluation=np.ones((N, A, 1), np.uint8), on_reset=g[pre + "on_reset"]), N


def test_attention_rollout_golden_and_checkpoint_round_trip(golden):
    """[N, agents, ...] requests with nested observations on the trained weights, loaded under the reference's key names."""
    g = golden("steps_smac_attn.npz")
    pol = policy_api.make(config.Policy("smac_rnn", args=dict(POLICY, seed=5)))
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in state_dict(g, "step1").items()}
    pol.load_checkpoint({"steps": 2, "state_dict": sd})
    back = pol.get_checkpoint()
    assert back["steps"] == 2 and list(back["state_dict"])[:2] == ["actor_base.obs_self_norm.weight", "actor_base.obs_self_norm.bias"]
    for k, v in sd.items():
        assert np.array_equal(back["state_dict"][k].numpy(), v.numpy()), k
    req, N = roll_request(g)
    res = pol.rollout(req)
    assert res.action.x.shape == (N, A, 1) and np.array_equal(res.action.x, g["roll_action"])
    assert close(res.analyzed_result.log_probs, g["roll_log_probs"], 1e-5)
    assert close(res.analyzed_result.value, g["roll_value"], 1e-5)
    assert close(res.policy_state.actor_hx, g["roll_new_actor_hx"], 1e-5)
    assert close(res.policy_state.critic_hx, g["roll_new_critic_hx"], 1e-5)
    with pytest.raises(KeyError):   # a missing leaf is an error, not a silent default
        bad = NamedArray(**{k: v for k, v in req.obs.items() if k != "local_obs"},
                         local_obs=NamedArray(**{k: v for k, v in req.obs.local_obs.items() if k != "obs_move"}))
        pol.rollout(policy_api.RolloutRequest(obs=bad, policy_state=None, is_evaluation=np.ones((N, 1), np.uint8),
                                              on_reset=np.ones((N, A, 1), np.uint8)))


def test_mixed_attention_obs_flat_state_analyze(golden):
    g = golden("steps_smac_attn.npz")
    pol = policy_api.make(config.Policy("smac_rnn", args=MIXED_POLICY))
    pol.load_checkpoint({"steps": 0, "state_dict": {k: torch.from_numpy(np.asarray(v)) for k, v in state_dict(g, "mixed_init").items()}})
    sample, arrays = make_sample(g, 0, state=g["mixed_state"])
    Tb = arrays["on_reset"].shape[0]
    ar = pol.analyze(sample[:Tb - 1], target="ppo")
    dead = arrays["obs.is_alive"][:Tb - 1] == 0
    lp = ar.new_action_log_probs.cpu().numpy()
    assert np.array_equal(np.isneginf(lp), dead)
    assert close(lp[~dead], g["mixed_new_lp"][~dead], 1e-5)
    assert close(ar.state_values.cpu().numpy(), g["mixed_value"], 1e-5)
    assert close(ar.entropy.cpu().numpy(), g["mixed_entropy"], 1e-5)


def test_fused_dense_tail_equals_layer_by_layer():
    """From 512 rows the dense tail behind the block runs as one launch per direction (and hands the block its gradient); forced
    layer by layer, the same update must come out.  600 rows: more than one tile per workgroup, a ragged last tile.
    The bound on the parameters is that of test_gpu_smac.py::test_encoder_pieces_do_not_change_the_step, for its reason: the first
    Adam step moves a weight by lr * g / (|g| + eps), so where |g| ~ eps = 1e-5 the two paths' rounding noise in g becomes a
    fraction of lr = 5e-4 (the cap), and everywhere else -- all but a thousandth of the elements -- they agree to 1e-6."""
    rng = np.random.default_rng(3)
    sample_kw = dict(SAMPLE, T=20, B=10)
    arrays = synthetic.make_multiagent_arrays(seed=11, **sample_kw)
    arrays.pop("obs.local_obs")
    lead = arrays["on_reset"].shape[:3]
    tree = {}
    for top, shapes in (("local_obs", POLICY["obs_shape"]), ("state", POLICY["state_shape"])):
        leaves = {}
        for k, shp in shapes.items():
            leaves[k] = ((rng.random((*lead, *shp)) < 0.7).astype(np.float32) if k.endswith("_mask") else
                         rng.standard_normal((*lead, *shp)).astype(np.float32))
        tree[top] = NamedArray(**leaves)
    results = []
    for fused in (True, False):
        trainer = trainer_api.make(config.Trainer("mappo", args=dict(TRAINER, ppo_epochs=1)), config.Policy("smac_rnn", args=POLICY))
        trainer.policy.net._enc_fused = fused
        sample = synthetic.to_sample_batch({k: v.copy() for k, v in arrays.items()})
        sample.obs = NamedArray(available_action=arrays["obs.available_action"], is_alive=arrays["obs.is_alive"], **tree)
        res = trainer.step(sample)
        results.append((res.stats, trainer.policy.net.flat.clone()))
    for k in ("policy_loss", "value_loss", "entropy", "grad_norm"):
        assert abs(results[0][0][k] - results[1][0][k]) <= 1e-6 * max(1.0, abs(results[1][0][k])), (k, results[0][0][k], results[1][0][k])
    d = (results[0][1] - results[1][1]).abs()
    assert float(d.max()) <= 5e-4 and float((d > 1e-6).float().mean()) < 1e-3, (float(d.max()), float((d > 1e-6).float().mean()))


def test_attention_step_replays_from_a_captured_graph(golden):
    """use_graph=True: the block's launches take their descriptor by value and neither allocate nor synchronise, so the step's device
    part is captured once and replayed; replayed steps equal eager ones (tolerances of test_gpu_graph.py)."""
    g = golden("steps_smac_attn.npz")
    mk = lambda graph: trainer_api.make(config.Trainer("mappo", args=dict(TRAINER, use_graph=graph)), config.Policy("smac_rnn", args=POLICY))
    eager, graphed = mk(False), mk(True)
    for step in range(4):  # step 0 eager in both, step 1 captures, steps 2.. replay
        (sa, _), (sb, _) = make_sample(g, step % 2), make_sample(g, step % 2)
        ra, rb = eager.step(sa), graphed.step(sb)
        for k, v in ra.stats.items():
            assert abs(v - rb.stats[k]) <= 2e-5 * max(1.0, abs(v)), (step, k, v, rb.stats[k])
        assert np.allclose(sa.analyzed_result.adv, sb.analyzed_result.adv, rtol=1e-6, atol=1e-7)
    pa, pb = eager.get_checkpoint(), graphed.get_checkpoint()
    for k in pa["state_dict"]:
        assert torch.allclose(pa["state_dict"][k], pb["state_dict"][k], rtol=0, atol=1e-5), k
    assert len(graphed._graphs) == 1 and next(iter(graphed._graphs.values())) is not None
