"""The fused recurrent step (csrc/rnn_step.hip) against the two-launch path (srl_gemm + cell, `hip.RNN_STEP_FUSED` cleared), on one GPU.

  * ``rnnpath``'s forward time loop over C = 40 steps, each path named: GRU and LSTM at H = 512 with N = 128 rows per step (the
    recurrent atari-dqn agent at 64 environments, two chunks) and at H = 128 with N = 256 (the football / overcooked width);
    device events around 10 loops, 9 repetitions, the two ways alternating; microseconds per loop, median / min / max;
  * one ``q-learning`` update of the recurrent ``atari-dqn`` agent (GRU, hidden_dim 512, chunk_len 40, burn_in_steps 40, B = 64;
    120 x 64 frames), host clock around the synchronised step, the two ways alternating; milliseconds.
Prints one JSON line per case and, with ``--out FILE``, writes them all (DESIGN.md / LAB_NOTEBOOK section 19 quote a run of it).

    python scripts/rnn_step_bench.py [--out rnn_step_bench.json]
"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import srl_amd
from srl_amd import hip
from srl_amd.algorithm.rnnpath import CELLS, bufs_of

DEV = "cuda:0"
srl_amd.register_all()
out = {}


def loop_case(kind, H, N, C=40, reps=9, inner=10):
    G = 4 if kind == "lstm" else 3
    g = torch.Generator().manual_seed(1)
    rn = lambda *s: torch.randn(*s, generator=g).to(DEV)
    w, b = rn(G * H, H) / H ** 0.5, 0.1 * rn(G * H)
    pre0 = rn(C, N, G * H)
    pre, gh, hin, cin, y, cnew = pre0.clone(), rn(C, N, 3 * H), rn(C, N, H), rn(C, N, H), rn(C, N, H), rn(C, N, H)
    rs = (torch.rand(C, N, generator=g) < 0.1).to(torch.uint8).to(DEV)
    rp = lambda c: rs.data_ptr() + c * N
    k = CELLS[kind]
    s = bufs_of(kind, gi=pre, gh=gh, hin=hin, cin=cin, cnew=cnew, y=y)

    def run(fused):   # the product's forward time loop, the path named
        k.fwd(s, w.data_ptr(), b.data_ptr(), rp, N, H, C, path="fused" if fused else "cell")

    # results agree (same inputs): y of both ways
    ys = {}
    for fused in (False, True):
        pre.copy_(pre0)
        run(fused)
        torch.cuda.synchronize()
        ys[fused] = y.clone()
    diff = float((ys[True] - ys[False]).abs().max())
    times = {False: [], True: []}
    for fused in (False, True):   # warm up
        for _ in range(3):
            run(fused)
    torch.cuda.synchronize()
    for _ in range(reps):
        for fused in (False, True):
            pre.copy_(pre0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                run(fused)
            e1.record()
            torch.cuda.synchronize()
            times[fused].append(e0.elapsed_time(e1) / inner * 1e3)   # us per loop of C steps
    rec = {("fused" if k else "two_launch"): dict(median_us=statistics.median(v), min_us=min(v), max_us=max(v)) for k, v in times.items()}
    rec["max_abs_y_diff"] = diff
    out[f"{kind}_H{H}_N{N}_C{C}"] = rec
    print(kind, H, N, json.dumps(rec), flush=True)


def update_case(reps=5):
    from srl_amd.api import config, trainer as trainer_api
    from srl_amd.api.env_utils import DiscreteAction
    from srl_amd.api.trainer import SampleBatch
    from srl_amd.algorithm.dqn_policy import DQNPolicyState
    from srl_amd.namedarray import NamedArray
    from srl_amd.runtime import synthetic
    B, burn, cl, boot = 64, 40, 40, 5
    Tb = burn + 2 * cl
    pargs = dict(act_dim=6, dueling=True, chunk_len=cl, seed=1, hidden_dim=512, num_rnn_layers=1, rnn_type="gru")
    targs = dict(bootstrap_steps=boot, burn_in_steps=burn, use_soft_update=True, max_grad_norm=40.0)
    a = synthetic.make_sample_arrays(seed=1, T=Tb - boot, B=B, obs_spec={"obs": ((4, 84, 84), "u8")}, action_dims=6, p_done=0.02,
                                     bootstrap_steps=boot, policy_state={"hx": (1, 512)})
    dev = lambda x: torch.from_numpy(x).to(DEV)
    sample = SampleBatch(obs=NamedArray(obs=dev(a["obs.obs"])),
                         policy_state=DQNPolicyState(hx=dev(a["policy_state.hx"]), epsilon=np.ones((Tb, B, 1), np.float32)),
                         on_reset=dev(a["on_reset"]), done=dev(a["done"]), truncated=dev(a["truncated"]), action=DiscreteAction(dev(a["action.x"])),
                         reward=dev(a["reward"]), info_mask=a["info_mask"])
    trainer = trainer_api.make(config.Trainer("q-learning", args=targs), config.Policy("atari-dqn", args=pargs))
    times = {"0": [], "1": []}
    for mode in ("0", "1"):
        hip.RNN_STEP_FUSED = mode == "1"
        trainer.step(sample)
    torch.cuda.synchronize()
    import time
    for _ in range(reps):
        for mode in ("0", "1"):
            hip.RNN_STEP_FUSED = mode == "1"
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            trainer.step(sample)   # ends in a device-to-host copy of the statistics
            torch.cuda.synchronize()
            times[mode].append((time.perf_counter() - t0) * 1e3)
    rec = {("fused" if k == "1" else "two_launch"): dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v)) for k, v in times.items()}
    out["qlearning_update_gru512_B64_burn40_chunk40"] = rec
    print("update", json.dumps(rec), flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available()
    loop_case("gru", 512, 128)
    loop_case("lstm", 512, 128)
    loop_case("gru", 128, 256)
    loop_case("lstm", 128, 256)
    update_case()
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump(out, f, indent=1)
