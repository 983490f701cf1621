"""One full update of bench.py's Atari policy with the full action set (action_dim = 18: 18 + 1 head outputs behind LayerNorm(512))
with the closing LayerNorm + heads on the wide fused pair (HipNet.LNHEADS_WIDE = True) and layer by layer (False): ms per update
by HIP events, the two settings interleaved on one sample in one process.
    python scripts/ln_heads_wide_ab.py [--envs 4096] [--rollout-len 128] [--chunk-rows 16384] [--steps 5] [--rounds 3]"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
import srl_amd
from srl_amd import hip
from srl_amd.algorithm.hipnet import HipNet
from srl_amd.api import config, trainer as trainer_api

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--rollout-len", type=int, default=128)
ap.add_argument("--chunk-rows", type=int, default=16384)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--rounds", type=int, default=3)
args = ap.parse_args()
srl_amd.register_all()
sample = bench.device_sample(0, args.rollout_len, args.envs, "cuda:0")   # (its actions, drawn from 6, are valid among 18)
trainers = {}
for wide in (True, False):
    HipNet.LNHEADS_WIDE = wide
    trainers[wide] = trainer_api.make(config.Trainer("mappo", args=dict(bench.TRAINER, chunk_rows=args.chunk_rows)),
                                      config.Policy("actor-critic", args=dict(bench.POLICY, action_dim=18)))
    hip.dispatch_tiles(reset=True)
    for _ in range(3):
        trainers[wide].step(sample)
times = {True: [], False: []}
for _ in range(args.rounds):
    for wide in (True, False):
        HipNet.LNHEADS_WIDE = wide
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); a.record()
        for _ in range(args.steps):
            trainers[wide].step(sample)
        e.record(); torch.cuda.synchronize()
        times[wide].append(a.elapsed_time(e) / args.steps)
for wide in (True, False):
    print(f"LNHEADS_WIDE={wide}: ms per update " + " ".join(f"{t:.2f}" for t in times[wide]) + f"  (min {min(times[wide]):.2f})")
