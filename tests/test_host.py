"""Host-side pieces: plugin registries, sample types, TrajGAE, buffer stacking, batcher, parameter table, envs,
and the C-ABI library's symbol table (no compute calls: there is no GPU here)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import srl_amd
from srl_amd import hip
from srl_amd.algorithm import netspec as ns
from srl_amd.algorithm.ppo_types import PPORolloutAnalyzedResult
from srl_amd.api import config, environment, policy as policy_api, trainer as trainer_api
from srl_amd.api.env_utils import DiscreteAction, DiscreteActionSpace
from srl_amd.namedarray import NamedArray
from srl_amd.runtime import synthetic
from srl_amd.runtime.batcher import InferenceBatcher
from srl_amd.runtime.buffer import PriorityQueueBuffer

srl_amd.register_all()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_registries_use_reference_names():
    assert {"actor-critic", "actor-critic-separate", "actor-critic-shared", "actor-critic-auxiliary"} <= set(policy_api.ALL_POLICY_CLASSES)
    assert {"mappo", "mappg"} <= set(trainer_api.ALL_TRAINER_CLASSES)
    assert {"gae", "null"} <= set(trainer_api.ALL_TRAJ_POSTPROCESSOR_CLASSES)
    with pytest.raises(KeyError):
        environment.register("cartpole", object)


def test_cabi_library_exports_every_declared_symbol():
    """The binding's table comes from the header (srl_amd/cabi.py), so the library is what it is compared with: every parsed
    prototype resolves in it, and -- where `nm` is installed -- it defines no srl_* symbol the header does not declare."""
    header = open(os.path.join(ROOT, "include", "srl_hip.h")).read()
    declared = set(re.findall(r"\b(srl_[a-z0-9_]+)\s*\(", header))
    assert declared == set(hip.EXPORTED_SYMBOLS), declared ^ set(hip.EXPORTED_SYMBOLS)  # no prototype slipped past the parser
    lib = ctypes.CDLL(hip.library_path())
    for name in hip.EXPORTED_SYMBOLS:
        assert hasattr(lib, name), name
    nm = shutil.which("nm")
    if nm is None:
        print("note: `nm` not found -- library symbols the header does not declare were NOT looked for")
    else:
        out = subprocess.run([nm, "-D", "--defined-only", hip.library_path()], check=True, capture_output=True, text=True).stdout
        defined = {ln.split()[-1].split("@")[0] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("srl_")}
        assert defined == set(hip.EXPORTED_SYMBOLS), defined ^ set(hip.EXPORTED_SYMBOLS)
    assert hip.lib().srl_abi_version() == hip.ABI_VERSION
    # struct layouts the binding assumes (every struct, field by field, against a compiler: tests/test_cabi.py)
    assert ctypes.sizeof(hip.PpoHparams) == 44 and ctypes.sizeof(hip.GemmDesc) == 208


def test_product_path_fails_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    tr = trainer_api.make(config.Trainer("mappo", args=dict(popart=False)),
                          config.Policy("actor-critic", args=dict(obs_dim=4, action_dim=2, hidden_dim=16,
                                                                    num_dense_layers=1, num_rnn_layers=0, popart=False)))
    sample = synthetic.to_sample_batch(
        synthetic.make_sample_arrays(seed=0, T=4, B=2, obs_spec=synthetic.CARTPOLE_OBS, action_dims=2))
    with pytest.raises(hip.HipError):
        tr.step(sample)
    with pytest.raises(hip.HipError):
        tr.policy.rollout(policy_api.RolloutRequest(obs=NamedArray(obs=np.zeros((3, 4), np.float32))))


def test_unsupported_configs_raise():
    base = dict(obs_dim=4, action_dim=2, num_rnn_layers=0, popart=False)
    for bad in (dict(num_rnn_layers=1, rnn_type="gtrxl"), dict(continuous_action=True, std_type="state_dependent"),
                dict(auxiliary_head=True, shared_backbone=True),  # actor_critic_policy.py:196-197: the auxiliary head needs separate trunks
                dict(obs_dim={"o": (3, 10, 4, 4, 4)}),
                dict(obs_dim={"o": (3, 12, 12)}, cnn_layers=dict(o=[(4, 3, 1, 1, "mirror")])),
                dict(obs_dim={"o": (3, 4, 4)}, cnn_layers=dict(o=[(4, 3, 1, 4, "reflect")]))):
        with pytest.raises((NotImplementedError, AttributeError, ValueError)):
            policy_api.make(config.Policy("actor-critic", args={**base, **bad}))


def test_conv_encoder_param_tables_by_rank(golden):
    """Conv1d / Conv2d (padding, pooling) / Conv3d encoders: the reference's state_dict keys -- the pooling layers shift
    the indices inside nn.Sequential (modules/cnn.py:99-126) -- shapes, and layout round trips of every parameter."""
    for fname, tag, pargs in (("steps_cnn_nd.npz", "cnn1d", dict(obs_dim={"seq": (3, 59)}, action_dim=4, hidden_dim=16,
                                                                  num_dense_layers=1, num_rnn_layers=0, popart=False, layernorm=True,
                                                                  shared_backbone=True, seed=73, use_maxpool=dict(seq=True),
                                                                  cnn_layers=dict(seq=[(4, 3, 1, 0, 'zeros'), (8, 3, 2, 1, 'zeros'),
                                                                                       (4, 3, 1, 0, 'zeros')]))),
                              ("steps_cnn_nd.npz", "cnn3d", dict(obs_dim={"vol": (2, 9, 8, 7), "vec": 3}, action_dim=[2, 3],
                                                                  hidden_dim=16, num_dense_layers=1, num_rnn_layers=0, popart=False,
                                                                  layernorm=False, shared_backbone=False, seed=74, activation="tanh",
                                                                  use_maxpool=dict(vol=True),
                                                                  cnn_layers=dict(vol=[(4, 3, 1, 1, 'zeros'), (4, 2, 1, 0, 'zeros')])))):
        g = golden(fname)
        spec, vals = ns.build_netspec(**pargs)
        ref = {k[len(f"{tag}_init_param:"):]: g[k] for k in g.files if k.startswith(f"{tag}_init_param:")}
        assert sorted(ref) == sorted(vals)
        for info in spec.params.values():
            v = vals[info.key]
            assert tuple(v.shape) == ref[info.key].shape == info.ref_shape, info.key
            assert np.allclose(v.numpy(), ref[info.key], rtol=1e-4, atol=1e-4), info.key
            assert torch.equal(info.to_reference(info.to_internal(v)), v), info.key


def test_popart_param_table_and_init(golden):
    """PopArt head: the reference's state_dict keys (name-mangled parameters + float64 running statistics), the
    nn.Linear default reset instead of the orthogonal one, same seed -> same initial weights."""
    g = golden("steps_popart.npz")
    c1 = dict(obs_dim=4, action_dim=2, hidden_dim=64, num_dense_layers=2, num_rnn_layers=0, popart=True, layernorm=False,
              shared_backbone=False, seed=7)
    spec, vals = ns.build_netspec(**c1)
    assert spec.popart and list(vals)[-5:] == [ns.POPART_W, ns.POPART_B, *ns.POPART_KEYS]
    ref_keys = [k[len("pa_init_param:"):] for k in g.files if k.startswith("pa_init_param:")]
    assert sorted(ref_keys) == sorted(vals)
    for k, v in vals.items():
        assert v.dtype == (torch.float64 if "_RunningMeanStd__" in k else torch.float32)
        assert np.allclose(v.numpy(), g[f"pa_init_param:{k}"], rtol=1e-4, atol=1e-4), k


def test_param_table_layout_roundtrip_and_init_sha(golden):
    import hashlib
    cnn = dict(obs_dim={"obs": (4, 84, 84)}, action_dim=6, hidden_dim=512, num_dense_layers=0, num_rnn_layers=0,
               popart=False, layernorm=False, shared_backbone=True, seed=5,
               cnn_layers=dict(obs=[(32, 8, 4, 0, 'zeros'), (64, 4, 2, 0, 'zeros'), (64, 3, 1, 0, 'zeros')]))
    spec, vals = ns.build_netspec(**cnn)
    assert sum(p.numel for p in spec.params.values()) == 1745191  # SURVEY.md 2.1 (measured on the reference)
    h = hashlib.sha256()
    for k, v in vals.items():
        h.update(k.encode())
        h.update(np.ascontiguousarray(v.numpy()).tobytes())
    if h.hexdigest() != str(golden("steps_cnn.npz")["cnn_init_sha"]):
        # LAPACK's QR (inside orthogonal_) can round differently on another CPU; bit-equality with the reference
        # was asserted where the fixtures were generated (tests/golden/gen_golden.py: check_init)
        print("note: initial weights differ in the last bits from the recorded reference run")
    g = golden("steps_mlp.npz")
    c1 = dict(obs_dim=4, action_dim=2, hidden_dim=64, num_dense_layers=2, num_rnn_layers=0, popart=False, layernorm=False,
              shared_backbone=False, seed=1)
    for k, v in ns.build_netspec(**c1)[1].items():
        assert np.allclose(v.numpy(), g[f"c1_init_param:{k}"], rtol=1e-5, atol=1e-6), k
    for name, info in spec.params.items():
        assert info.offset % 4 == 0
        back = info.to_reference(info.to_internal(vals[name]))
        assert torch.equal(back, vals[name]), name
    w = vals["obs_modules_dict.obs.1._Convolution__model.2.weight"]
    info = spec.params["obs_modules_dict.obs.1._Convolution__model.2.weight"]
    assert info.layout == "conv_nhwc"
    assert torch.equal(info.to_internal(w).reshape(64, 4, 4, 32)[3, 1, 2, 5], w[3, 5, 1, 2])
    fc = spec.params["obs_modules_dict.obs.1._Convolution__model.7.0.weight"]
    assert fc.layout == "fc_from_chw" and fc.chw == (64, 7, 7)
    pol = policy_api.make(config.Policy("actor-critic", args=cnn))
    sd = pol.get_checkpoint()["state_dict"]
    assert list(sd) == list(vals) and all(torch.equal(sd[k], vals[k]) for k in sd)
    pol.load_checkpoint({"steps": 7, "state_dict": {k: v + 1 for k, v in sd.items()}})
    assert pol.version == 7 and torch.equal(pol.get_checkpoint()["state_dict"]["actor_head.bias"], sd["actor_head.bias"] + 1)


def test_traj_gae_postprocessor(golden):
    g = golden("host.npz")
    for tag in ("trunc", "done"):
        rew, value, done, trunc = g[f"trajgae_{tag}_in"]
        memory = [
            trainer_api.SampleBatch(obs=None, reward=np.array([r], np.float32),
                                    analyzed_result=PPORolloutAnalyzedResult(value=np.array([v], np.float32),
                                                                             log_probs=None),
                                    done=np.array([d]), truncated=np.array([t]))
            for r, v, d, t in zip(rew, value, done, trunc)
        ]
        proc = trainer_api.make_traj_postprocessor(config.TrajPostprocessor('gae', args=dict(gamma=0.1, lmbda=0.1)))
        memory = proc.process(memory)
        np.testing.assert_allclose([m.analyzed_result.adv.item() for m in memory[:-1]], g[f"trajgae_{tag}_adv"], rtol=1e-6)
        np.testing.assert_allclose([m.analyzed_result.ret.item() for m in memory[:-1]], g[f"trajgae_{tag}_ret"], rtol=1e-6)


def test_buffer_stacks_on_axis_one_like_reference(golden):
    g = golden("host.npz")
    buf = PriorityQueueBuffer(max_size=4, reuses=2, batch_size=3)
    for i in range(3):
        arr = synthetic.make_sample_arrays(seed=40 + i, T=4, B=1, obs_spec=synthetic.CARTPOLE_OBS, action_dims=2)
        arr = {k: v[:, 0] for k, v in arr.items()}
        assert np.array_equal(arr["obs.obs"], g[f"buffer_in{i}_obs"])
        formed = buf.put(synthetic.to_sample_batch(arr))
        assert formed == (i == 2)
    e = buf.get()
    assert np.array_equal(e.sample.obs.obs, g["buffer_obs"]) and np.array_equal(e.sample.reward, g["buffer_reward"])
    assert np.array_equal(e.sample.action.x, g["buffer_action"])
    assert e.sample.obs.obs.shape == (5, 3, 4) and e.reuses_left == 1 and buf.qsize() == 1  # served twice
    buf.get()
    assert buf.empty()


class _EchoPolicy(policy_api.Policy):
    """Counts rows per call; action = row index so the batcher's slicing can be checked."""

    def __init__(self):
        self.device = "cpu"
        self.calls = []
        self._version = 3

    @property
    def version(self):
        return self._version

    def load_checkpoint(self, ckpt):
        self._version = ckpt["steps"]

    def rollout(self, requests, **kw):
        n = requests.length(dim=0)
        self.calls.append(n)
        return policy_api.RolloutResult(action=DiscreteAction(requests.obs.obs[:, :1].astype(np.int64)),
                                        analyzed_result=PPORolloutAnalyzedResult(log_probs=np.zeros((n, 1), np.float32),
                                                                                 value=np.zeros((n, 1), np.float32)))


def _req(ids):
    ids = np.asarray(ids)
    n = len(ids)
    return policy_api.RolloutRequest(obs=NamedArray(obs=np.repeat(ids[:, None], 4, 1).astype(np.float32)),
                                     is_evaluation=np.zeros((n, 1), np.uint8), on_reset=np.zeros((n, 1), np.uint8),
                                     step_count=np.zeros((n, 1), np.int32), client_id=ids[:, None].astype(np.int32),
                                     request_id=(ids[:, None] * 10).astype(np.int32),
                                     received_time=np.zeros((n, 1), np.int64), buffer_index=np.zeros((n, 1), np.int32),
                                     ready=np.zeros((n, 1), np.bool_))


def test_inference_batcher_merges_caps_and_stamps():
    pol = _EchoPolicy()
    ckpts = [dict(steps=9)]
    b = InferenceBatcher(pol, policy_name="p", batch_size=5, parameter_source=lambda: ckpts.pop() if ckpts else None)
    b.post(_req([0, 1]))
    b.post(_req([2]))
    assert b.batch_step() == 2  # 3 rows queued, not yet run
    b.post(_req([3, 4, 5, 6]))
    assert b.batch_step() == 1  # merged with the un-started batch: 7 rows -> 5 go, 2 carried
    res = b.inference()
    assert pol.calls == [5] and pol.version == 9
    assert np.array_equal(res.client_id[:, 0], [0, 1, 2, 3, 4]) and np.array_equal(res.request_id[:, 0], [0, 10, 20, 30, 40])
    assert np.array_equal(res.action.x[:, 0], [0, 1, 2, 3, 4])
    assert (res.policy_version_steps == 9).all() and (res.policy_name == "p").all() and res.ready.all()
    rest = b.poll()
    assert pol.calls == [5, 2] and np.array_equal(rest[0].client_id[:, 0], [5, 6]) and b.pending_rows() == 0


def test_environments_follow_step_contract():
    for name, shape in (("cartpole", (4,)), ("synthetic-atari", (4, 84, 84))):
        env = environment.make(config.Environment(name, args=dict(seed=1)))
        assert env.agent_count == 1
        [r] = env.reset()
        assert r.obs["obs"].shape == shape and r.done.dtype == np.uint8 and r.reward.shape == (1,)
        for _ in range(5):
            [r] = env.step([env.action_spaces[0].sample()])
            assert r.reward.dtype == np.float32 and r.truncated.shape == (1,) and r.done.shape == (1,)
            assert not (r.done[0] and r.truncated[0])
    sp = DiscreteActionSpace([3, 4], seed=0)
    assert sp.sample().x.shape == (2,)
    avail = np.array([0, 0, 1, 0, 0, 0], bool)
    assert DiscreteActionSpace(6, seed=0).sample(avail).x[0] == 2


def test_synthetic_sample_obeys_reference_invariants():
    a = synthetic.make_sample_arrays(seed=3, T=64, B=16, obs_spec=synthetic.CARTPOLE_OBS, action_dims=[3, 2], p_done=0.2)
    done, trunc, orr = (a[k].astype(np.float64) for k in ("done", "truncated", "on_reset"))
    assert (trunc * done == 0).all() and ((trunc + done)[:-1] == orr[1:]).all()  # gae.py:69-70
    assert (a["reward"][:-1] * orr[1:] == 0).all() and (a["analyzed_result.value"] * done == 0).all()  # :72, mappo.py:124
    assert a["action.x"].shape == (65, 16, 2) and a["done"].dtype == np.uint8 and a["action.x"].dtype == np.int32


def test_executor_host_logic_of_round_3():
    """Host-side decisions of the executor that need no GPU: split-K factors of weight gradients, and the validity window of
    what an executor derives from the weights (only inside the trainer's chunk loop, only for the current parameter version,
    only for the same buffer; the record is keyed by the buffer and shared with the twins, whose own buffers are other
    pointers, while the weight-only data of the two-piece block lives in the first executor's workspace for all of them)."""
    from srl_amd.algorithm import hipnet
    assert hipnet._split_for(256, 1) == 1            # CartPole-sized: one piece (srl_gemm's small-product path)
    assert hipnet._split_for(16384, 1) == 32         # >= 512 rows per slice
    assert hipnet._split_for(16384, 100) == 5        # enough workgroups already
    spec, vals = ns.build_netspec(obs_dim=4, action_dim=2, hidden_dim=8, num_dense_layers=1, num_rnn_layers=0, popart=False,
                                  layernorm=False, shared_backbone=False, seed=1)
    net = hipnet.HipNet(spec, "cpu")
    assert not net._derived_fresh("w", 1000)         # outside an update: never cached
    assert not net._derived_fresh("w", 1000)
    net.chunks_of_one_update(True)
    assert not net._derived_fresh("w", 1000)         # first chunk computes ...
    assert net._derived_fresh("w", 1000)             # ... the following ones reuse
    assert not net._derived_fresh("w", 2000)         # another buffer (outgrown workspace): recompute
    twin = net.twin()
    assert twin.wws is net.ws and twin.ws is not net.ws   # one set of derived weights, a workspace of its own for the rest
    assert twin._derived_fresh("w", 2000)            # a SHARED buffer the first executor filled: fresh for the twin
    assert not twin._derived_fresh("w", 3000)        # a buffer of the twin's own workspace holds nothing yet
    assert twin._derived_fresh("w", 3000)
    net.params_changed()                             # optimiser step: everything derived is stale, for the twin too
    assert not net._derived_fresh("w", 2000) and not twin._derived_fresh("w", 3000)
    assert twin._derived_fresh("w", 2000)            # ... and recomputed by one of them for both
    net.chunks_of_one_update(False)
    assert not net._derived_fresh("w", 2000) and not twin._derived_fresh("w", 3000)


def _net_and_twins():
    from srl_amd.algorithm import hipnet
    spec, _ = ns.build_netspec(obs_dim=4, action_dim=2, hidden_dim=8, num_dense_layers=1, num_rnn_layers=0, popart=True,
                               layernorm=False, shared_backbone=False, seed=1)
    net = hipnet.HipNet(spec, "cpu")
    return net, [net.twin(), net.twin()]


def test_twins_own_their_state_and_share_one_param_state():
    """An executor and its twins hold ONE `ParamState` (parameters, PopArt statistics, the weight-only workspace of the first
    executor); every other container, workspace or tensor of an executor is its own object."""
    from srl_amd.algorithm.hipnet import Workspace
    net, twins = _net_and_twins()
    shared_names = {"shared", "spec", "flat", "popart_state", "wws"}
    for twin in twins + [twins[0].twin()]:   # the last one: an executor made from a twin
        assert twin.shared is net.shared and twin.wws is net.ws and twin.ws is not net.ws
        assert twin.flat.data_ptr() == net.flat.data_ptr() and twin.popart_state.data_ptr() == net.popart_state.data_ptr()
        assert net.popart_state.numel() == 3 and twin.grad.data_ptr() != net.grad.data_ptr()
        assert vars(twin).keys() == vars(net).keys()
        for name, mine in vars(net).items():
            if isinstance(mine, (dict, list, set, Workspace, torch.Tensor)):
                assert (vars(twin)[name] is mine) == (name in shared_names), name
    assert net.shared.has_twins


def test_weight_range_slots_are_one_table_for_all_executors():
    """The host half of `_weight_range` (no launch: the refill is the caller's callback): slots and staleness live in the shared
    state, whichever executor allocates, invalidates or refills them."""
    net, (twin, _) = _net_and_twins()
    filled = []
    assert twin._weight_slot("a", filled.append) == 0 and net._weight_slot("b", filled.append) == 1
    assert net._weight_slot("a", filled.append) == 0 and filled == [0, 1]     # the twin's slot, already filled: no refill
    net.params_changed()
    assert net.shared.wamax_stale == twin.shared.wamax_stale == {"a", "b"}
    assert twin._weight_slot("b", filled.append) == 1 and filled == [0, 1, 1]  # refilled through the twin ...
    assert net._weight_slot("b", filled.append) == 1 and filled == [0, 1, 1]   # ... is current for the first executor
    assert net._weight_slot("a", filled.append) == 0 and filled == [0, 1, 1, 0]
    assert not net.shared.wamax_stale and net.refresh_weight_ranges() == 2
    for i in range(2, 256):
        assert twin._weight_slot(f"p{i}", filled.append) == i
    assert net._weight_slot("p256", filled.append) is None and twin._weight_slot("p256", filled.append) is None   # the 257th
    assert len(filled) == 258 and len(net.shared.wamax_slot) == 256 and not net.shared.wamax_stale


def test_update_and_serving_windows_are_seen_by_every_executor():
    net, (twin, _) = _net_and_twins()
    net.begin_serving()
    net.begin_serving()
    assert not net._derived_fresh("w", 1000) and twin._derived_fresh("w", 1000)
    net.end_serving()
    assert net._derived_fresh("w", 1000)                  # still serving: kept
    net.end_serving()
    assert not net._derived_fresh("w", 1000) and net.shared.serving == 0
    assert not net.in_update and not twin.in_update and net._presplit("k", 1024, 64, 0) is None
    net.chunks_of_one_update(True, pipelines=2)
    assert net.in_update and twin.in_update and twin.shared.multi
    assert net._presplit("k", 1024 + 4, 64, 0) is None and net._presplit("k", 1024, 63, 0) is None   # unaligned
    assert not net._derived_fresh("w", 1000) and net._derived_fresh("w", 1000)
    net._derived_forget(1000)
    assert not twin._derived_fresh("w", 1000)
    net.last_chunk = True
    net.chunks_of_one_update(False)
    assert not twin.in_update and not net.shared.multi and net.last_chunk is None
    net.chunks_of_one_update(True)
    assert net.in_update and not net.shared.multi      # (one pipeline: the trainers that never fork do not say how many)
    net.chunks_of_one_update(False)


def test_param_state_keeps_no_executor_alive():
    import gc
    import weakref
    net, twins = _net_and_twins()
    shared, first = net.shared, weakref.ref(net)
    del net, twins
    gc.collect()
    assert first() is None and shared.wws is not None


def test_host_side_queries_of_the_fused_kernels():
    """The planning queries the Python side makes before a launch are host code (no GPU): which (chain, rows) pairs keep no
    tape (srl_mlp_tape_floats_at -- the matrix-core chains walk forward again in their backward pass) and which LayerNorm + heads
    tails run as one launch (srl_ln_heads_supported)."""
    from srl_amd import hip
    chain = [(0, 4, 4, 0, 1, 1, 1, 1), (1, 4, 64, 1, 1, 1, 1, 1), (0, 64, 64, 0, 1, 1, 1, 1), (1, 64, 2, 0, 1, 1, 1, 1)]
    arr = hip.mlp_layers(chain)
    full = hip.mlp_tape_floats(arr)
    assert full == 4 + 64 + 64
    assert hip.mlp_tape_floats_at(arr, 511) == full        # the FMA chain keeps every layer's input
    assert hip.mlp_tape_floats_at(arr, 512) == 0           # the matrix-core chain keeps none
    wide = hip.mlp_layers([(1, 4, 128, 1, 1, 1, 1, 1), (1, 128, 2, 0, 1, 1, 1, 1)])
    assert hip.mlp_tape_floats_at(wide, 65536) == hip.mlp_tape_floats(wide) == 128   # wider than 64: not a matrix-core chain
    assert hip.ln_heads_supported(512, (6, 1)) and hip.ln_heads_supported(256, (8,)) and hip.ln_heads_supported(1024, (2, 1))
    assert not hip.ln_heads_supported(512, (8, 1))     # nine outputs
    assert not hip.ln_heads_supported(384, (6, 1)) and not hip.ln_heads_supported(512, ())


# every switch `srl_amd/` reads from the environment; a new one is added here and to INTEGRATION.md's table on purpose
ENV_SWITCHES = frozenset({
    "SRL_HIP_LIB", "SRL_COMM", "SRL_PIPELINES", "SRL_WGRAD_STREAM", "SRL_EXPLICIT_CONV", "SRL_H2", "SRL_FC_TRAIN_SPLITK",
    "SRL_OBS_BWD_DEFER", "SRL_RNN_SEQ", "SRL_MFMA", "SRL_F16X2", "SRL_OBS_BF16", "SRL_SMALL_GEMM", "SRL_MLP_F16", "SRL_MLP_SIG",
    "SRL_H2GEMM_P", "SRL_CONV_RUN_IMAGES"})


def test_environment_switches_match_the_documented_table():
    """The `SRL_*` names inside `os.environ...(` / `getenv(` calls of srl_amd/**/*.py and srl_amd/csrc/* are exactly the rows of
    INTEGRATION.md's switch table, and no more of them than the set above (source text only, nothing is launched)."""
    import glob
    paths = glob.glob(os.path.join(ROOT, "srl_amd", "**", "*.py"), recursive=True)
    paths += [p for p in glob.glob(os.path.join(ROOT, "srl_amd", "csrc", "*")) if p.endswith((".hip", ".h"))]
    read = set()
    for path in paths:
        read |= set(re.findall(r"(?:os\.environ[.\w]*[\[(]|getenv\()\s*[\"'](SRL_[A-Z0-9_]+)[\"']", open(path).read()))
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    table = doc[doc.index("Switches read from the environment"):]
    rows = [ln for ln in table[:table.index("\n\n", table.index("|---|"))].splitlines() if ln.startswith("| `")]
    documented = set()
    for ln in rows:
        documented |= set(re.findall(r"SRL_[A-Z0-9_]+", ln.split("|")[1]))
    assert read == documented, (sorted(read - documented), sorted(documented - read))
    assert read <= ENV_SWITCHES and len(read) <= len(ENV_SWITCHES), sorted(read - ENV_SWITCHES)


def test_every_layer_kind_has_its_forward_and_backward_handler():
    """The executor picks a forward handler by spec class and a backward handler by record kind (hipnet.HipNet.FWD_HANDLERS /
    BWD_HANDLERS).  Every layer descriptor of netspec -- its dataclasses that carry a parameter `prefix`; the containers
    (EncoderSpec, NetSpec, ParamInfo) carry none -- has a forward handler, every record kind a forward handler declares has a
    backward handler, and the kinds that release their own gradient buckets are kinds that exist."""
    import dataclasses
    import inspect
    from srl_amd.algorithm.hipnet import HipNet
    layer_specs = [c for _, c in inspect.getmembers(ns, inspect.isclass)
                   if c.__module__ == ns.__name__ and dataclasses.is_dataclass(c) and hasattr(c, "__dataclass_fields__")
                   and ("prefix" in c.__dataclass_fields__ or hasattr(c, "prefix"))]
    assert {ns.LinearSpec, ns.LayerNormSpec, ns.GruSpec, ns.ConvSpec, ns.InstrLstmSpec} <= set(layer_specs) and len(layer_specs) >= 10
    assert not {ns.EncoderSpec, ns.NetSpec, ns.ParamInfo} & set(layer_specs)
    missing = [c.__name__ for c in layer_specs if c not in HipNet.FWD_HANDLERS]
    assert not missing, f"no forward handler for {missing}"
    assert set(HipNet.FWD_HANDLERS) <= set(layer_specs)
    assert HipNet.FWD_KINDS and set(HipNet.FWD_KINDS) <= set(HipNet.BWD_HANDLERS), set(HipNet.FWD_KINDS) - set(HipNet.BWD_HANDLERS)
    assert set(HipNet.BWD_OWN_RELEASE) <= set(HipNet.BWD_HANDLERS)
    assert all(callable(f) for f in list(HipNet.FWD_HANDLERS.values()) + list(HipNet.BWD_HANDLERS.values()))


def test_chunk_major_decision_truth_table():
    """rnnpath.chunk_major(spec, rnn, obs): a whole pass runs on chunk-major rows for a recurrent net with more than one chunk and
    2-D contiguous float32 observations under every encoder key -- and for nothing else, one change at a time."""
    from srl_amd.algorithm.rnnpath import RnnCtx, chunk_major
    base = dict(obs_dim={"a": 5, "b": 3}, action_dim=2, hidden_dim=8, num_dense_layers=1, num_rnn_layers=1, popart=False,
                layernorm=True, shared_backbone=False)
    spec = lambda **kw: ns.build_netspec(**dict(base, **kw))[0]
    T, B, C = 8, 3, 4
    rnn = RnnCtx(T, B, C, {}, None)
    obs = {"a": torch.zeros(T * B, 5), "b": torch.zeros(T * B, 3)}
    assert chunk_major(spec(), rnn, obs) is True
    assert chunk_major(spec(shared_backbone=True), rnn, obs) is True
    assert chunk_major(spec(rnn_type="lstm", num_rnn_layers=2), rnn, obs) is True
    false_for = {
        "one chunk": (spec(), RnnCtx(C, 2 * B, C, {}, None), obs),
        "no recurrent layers": (spec(num_rnn_layers=0), rnn, obs),
        "no context": (spec(), None, obs),
        "shared_learnable": (spec(continuous_action=True, std_type="shared_learnable"), rnn, obs),
        "auxiliary value head": (spec(auxiliary_head=True), rnn, obs),
        "uint8 observation": (spec(), rnn, dict(obs, b=torch.zeros(T * B, 3, dtype=torch.uint8))),
        "3-D observation": (spec(), rnn, dict(obs, b=torch.zeros(T * B, 1, 3))),
        "non-contiguous view": (spec(), rnn, dict(obs, a=torch.zeros(T * B, 10)[:, ::2])),
        "missing key": (spec(), rnn, {"a": obs["a"]}),
    }
    assert chunk_major(spec(continuous_action=True, std_type="fixed"), rnn, obs) is True   # (only the shared log-sigma head refuses)
    for what, args in false_for.items():
        assert chunk_major(*args) is False, what
