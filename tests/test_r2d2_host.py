"""The recurrent ``atari-dqn`` agent (R2D2) without a GPU: the parameter table and seeded initial weights against the reference's
(tests/golden/r2d2.npz, written by tests/golden/gen_r2d2.py from the real reference), the internal layout of ``weight_ih_l0``,
checkpoint keys, ``default_policy_state``, the burn-in index arithmetic against a literal restatement of the reference's, the options
that stay refused, the fused step kernel's symbols, and the torch restatement tests/r2d2_ref.py pinned to the reference's recorded
run at hidden_dim 512 (the device tests use it as their oracle at the small widths)."""
import numpy as np
import pytest
import torch

import r2d2_ref
import srl_amd
from r2d2_cases import RUNS, TABLES, TABLE_STRIDE, bar_scale, e2e_arrays, rel_err
from srl_amd import hip
from srl_amd.algorithm import netspec as ns
from srl_amd.algorithm.dqn_policy import burn_in_plan
from srl_amd.api import config, policy as policy_api

srl_amd.register_all()
RNN = "rnn._AutoResetRNN__net."


@pytest.fixture(scope="module")
def g(golden):
    return golden("r2d2.npz")


@pytest.fixture(scope="module")
def policies():
    return {tag: policy_api.make(config.Policy("atari-dqn", args=args)) for tag, args in TABLES.items()}


@pytest.mark.parametrize("tag", list(TABLES))
def test_parameter_table_and_seeded_weights_equal_the_reference(g, policies, tag):
    sd = policies[tag].get_checkpoint()["state_dict"]
    names = [str(k) for k in g[f"table_{tag}_names"]]
    assert list(sd) == names
    assert [tuple(v.shape) for v in sd.values()] == [tuple(int(x) for x in s if x) for s in g[f"table_{tag}_shapes"]]
    samples = np.concatenate([v.numpy().reshape(-1)[::TABLE_STRIDE] for v in sd.values()])
    assert np.array_equal(samples, g[f"table_{tag}_samples"])
    # the recurrent parameters sit between the trunk and the towers, under both networks
    i = names.index("net." + RNN + "weight_ih_l0")
    assert names[i - 1] == "net.conv3.bias" and names[i + 4 * TABLES[tag]["num_rnn_layers"]] == "net.fc.0.weight"
    assert "target_net." + RNN + "bias_hh_l0" in names
    for k, v in sd.items():  # the target is a copy
        if k.startswith("net."):
            assert torch.equal(v, sd["target_" + k])


@pytest.mark.parametrize("tag", list(TABLES))
def test_default_policy_state(g, policies, tag):
    st = policies[tag].default_policy_state
    assert st.hx.shape == tuple(g[f"table_{tag}_default_hx_shape"]) and st.hx.dtype == np.float32 and not st.hx.any()
    assert st.epsilon.shape == (1,)


def test_weight_ih_l0_layout_round_trip():
    """The trunk's rows are NHWC, the reference flattens CHW: ``weight_ih_l0`` is stored with its columns permuted, as ``fc.0.weight``
    of the feed-forward agent is; the towers behind the recurrent layer are stored plain."""
    spec, _ = ns.build_atari_dqn_netspec(6, 8, num_rnn_layers=2, rnn_type="lstm")
    info = spec.params[RNN + "weight_ih_l0"]
    assert info.layout == "fc_from_chw" and info.chw == (64, 7, 7) and info.ref_shape == (32, 3136)
    assert spec.params[RNN + "weight_ih_l1"].layout == "plain" and spec.params["fc.0.weight"].layout == "plain"
    assert spec.params["fc.0.weight"].ref_shape == (8, 8)
    ref = torch.arange(32 * 3136, dtype=torch.float32).reshape(32, 3136)
    inner = info.to_internal(ref).reshape(32, 7, 7, 64)
    assert inner[3, 2, 5, 9] == ref[3, 9 * 49 + 2 * 7 + 5]   # column (c, h, w) of the reference at (h, w, c)
    assert torch.equal(info.to_reference(inner.reshape(-1)), ref)
    ff, _ = ns.build_atari_dqn_netspec(6, 8)
    assert ff.params["fc.0.weight"].layout == "fc_from_chw" and not ff.actor_backbone and ff.num_rnn_layers == 0


def literal_burn_in(rows, burn, chunk_len):
    """atari_dqn_policy.py:169-183, restated: the number of chunks and the slices ``_make_burn_in_data`` takes of the full sample."""
    sample_steps = rows - burn
    num_chunks = sample_steps // chunk_len
    return num_chunks, [(i * chunk_len, i * chunk_len + burn) for i in range(num_chunks)]


@pytest.mark.parametrize("rows,burn,cl", [(10, 2, 4), (12, 2, 4), (80, 40, 40), (84, 40, 40), (8, 0, 3), (6, 0, 3), (13, 3, 5)])
def test_burn_in_indices_are_the_reference_s(rows, burn, cl):
    plan = burn_in_plan(rows, burn, cl)
    K, windows = literal_burn_in(rows, burn, cl)
    assert plan.num_chunks == K and plan.chunk * K == rows - burn
    if burn:
        assert plan.windows == windows and plan.state_rows == [a for a, _ in windows]
        assert all(b <= rows for _, b in windows)
    else:
        assert plan.windows == [] and plan.state_rows == [k * plan.chunk for k in range(K)]   # to_chunk(x, K)[0]


def test_burn_in_windows_when_the_chunk_is_longer_than_chunk_len():
    """10 analysed steps, chunk_len 4: two chunks of 5 (rows [2, 7) and [7, 12) with two burn-in steps), but the windows stay at the
    reference's k * chunk_len: the second, rows [4, 6), does not end in front of its chunk."""
    plan = burn_in_plan(12, 2, 4)
    assert (plan.num_chunks, plan.chunk, plan.windows, plan.state_rows) == (2, 5, [(0, 2), (4, 6)], [0, 4])
    aligned = burn_in_plan(10, 2, 4)
    assert (aligned.num_chunks, aligned.chunk, aligned.windows) == (2, 4, [(0, 2), (4, 6)])   # chunk k = rows [2 + 4 k, 6 + 4 k)
    with pytest.raises(ValueError):
        burn_in_plan(13, 2, 4)   # 11 steps, two chunks
    with pytest.raises(ValueError):
        burn_in_plan(5, 2, 4)    # no chunk


def test_what_stays_refused_raises_at_construction():
    base = dict(act_dim=6, dueling=True, hidden_dim=16, num_rnn_layers=1, rnn_towers_read_hidden_dim=True)
    mk = lambda **kw: policy_api.make(config.Policy("atari-dqn", args=dict(base, **kw)))
    assert mk().spec.num_rnn_layers == 1
    for kw, word in ((dict(dueling=False), "dueling"), (dict(rnn_type="gtrxl"), "gtrxl"),
                     (dict(rnn_include_last_action=True), "rnn_include_last"), (dict(rnn_include_last_reward=True), "rnn_include_last")):
        with pytest.raises(NotImplementedError, match=word):
            mk(**kw)
    with pytest.raises(NotImplementedError, match="hidden_dim=512 only"):   # the reference's towers: no other width without the extension
        mk(rnn_towers_read_hidden_dim=False)
    assert policy_api.make(config.Policy("atari-dqn", args=dict(act_dim=6, dueling=True, hidden_dim=16))).spec.num_rnn_layers == 0
    with pytest.raises(NotImplementedError, match="multiple of 4"):
        mk(hidden_dim=18)
    import torch.distributed as dist
    dist.init_process_group("gloo", store=dist.HashStore(), rank=0, world_size=1)   # a process group of one, in this process
    try:
        with pytest.raises(NotImplementedError, match="data-parallel"):
            mk()
    finally:
        dist.destroy_process_group()


def test_fused_step_symbols_resolve():
    lib = hip.lib()
    for name in ("srl_rnn_step_supported", "srl_gru_step_fwd", "srl_lstm_step_fwd"):
        assert hasattr(lib, name), name
    for kind in ("gru", "lstm"):
        assert not hip.rnn_step_supported(kind, 64) and not hip.rnn_step_supported(kind, 520)   # the chunk kernel's; no multiple of 16
        assert hip.rnn_step_supported(kind, 512) and hip.rnn_step_supported(kind, 144)


@pytest.mark.parametrize("run", list(RUNS))
def test_restatement_equals_the_reference_at_512(g, run):
    """tests/r2d2_ref.py from this project's seeded initial weights (equal to the reference's, above) on the recorded sample of step
    0: ``q_tot`` and ``target_q_tot`` of the reference's ``analyze``, burn-in included, at the fixture's bar."""
    r = RUNS[run]
    sd = {k: v.numpy() for k, v in policy_api.make(config.Policy("atari-dqn", args=r["policy"])).get_checkpoint()["state_dict"].items()}
    torch.manual_seed(0)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        net, target = (r2d2_ref.make_net(sd, p, r["policy"], torch.float32) for p in ("net.", "target_net."))
        with torch.no_grad():
            out = r2d2_ref.analyze(net, target, e2e_arrays(run, 0), r["trainer"].get("burn_in_steps", 0), r["policy"]["chunk_len"], torch.float32)
    finally:
        torch.set_num_threads(threads)
    for k in ("q_tot", "target_q_tot"):
        err = rel_err(out[k].numpy(), g[f"{run}_{k}"], 1e-3)
        print(f"{run} {k}: {err:.2e} (bar {1e-5 * bar_scale(g, run, k):.2e})")
        assert out[k].shape == g[f"{run}_{k}"].shape and err <= 1e-5 * bar_scale(g, run, k), (k, err)
