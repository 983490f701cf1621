"""Prioritised replay at R2D2 shapes: the gather against its byte floor, and one get -> update_priorities round of the buffer resident
in HBM against the host buffer on the same box.

    python scripts/replay_bench.py [--max-size 256] [--tb 120] [--batch 64] [--rounds 30]

Prints one JSON line.
  gather_us        srl_replay_gather of the frame leaf alone ([Tb, B, 4 x 84 x 84] uint8), device events around 20 back-to-back calls,
                   median of 7 windows; gather_floor_us = one read + one write of the batch at 8 TB/s
  device_round_ms  DevicePrioritizedReplayBuffer: get (draws, weights, every leaf gathered) + update_priorities with device tensors,
                   host clock around `rounds` rounds that end in one synchronise
  host_round_ms    PrioritizedReplayBuffer: get (numpy fancy index of every leaf) + the upload of every leaf of the batch to the
                   device (what a trainer step does with a host sample) + update_priorities with numpy priorities, the same clock
The priorities handed back are random; no network runs between get and update_priorities in either round."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from srl_amd.api.env_utils import DiscreteAction
from srl_amd.api.trainer import SampleBatch
from srl_amd.namedarray import NamedArray, flatten
from srl_amd.runtime import synthetic
from srl_amd.runtime.buffer import make_buffer

HBM_BYTES_PER_S = 8e12


def actor_sample(k, tb):
    a = synthetic.make_sample_arrays(seed=k, T=tb - 2, B=1, obs_spec=synthetic.ATARI_OBS, action_dims=6, p_done=0.01, bootstrap_steps=2)
    a = {key: v[:, 0] for key, v in a.items()}
    return SampleBatch(obs=NamedArray(obs=a["obs.obs"]), on_reset=a["on_reset"], done=a["done"], truncated=a["truncated"],
                       action=DiscreteAction(a["action.x"]), reward=a["reward"], info_mask=a["info_mask"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-size", type=int, default=256)
    ap.add_argument("--tb", type=int, default=120)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=30)
    args = ap.parse_args()
    kw = dict(max_size=args.max_size, sample_length=args.tb, batch_size=args.batch, warmup_transitions=0, seed=1, alpha=0.6, beta=0.4)
    distinct = [actor_sample(k, args.tb) for k in range(8)]
    rng = np.random.default_rng(0)
    new_priorities = (rng.random((args.rounds + 3, args.batch)) * 2 + 0.01).astype(np.float32)

    host = make_buffer("prioritized_replay_buffer", **kw)
    for k in range(args.max_size):
        host.put(distinct[k % 8])

    import torch
    from srl_amd import hip
    hip.require_gpu()
    dev = make_buffer("prioritized_replay_buffer_hip", **kw)
    for k in range(args.max_size):
        dev.put(distinct[k % 8])
    dev_priorities = torch.from_numpy(new_priorities).cuda()

    def device_round(r):
        e = dev.get()
        dev.update_priorities(e.sampling_indices, dev_priorities[r])
        return e

    def host_round(r):
        e = host.get()
        leaves = [torch.from_numpy(v).to("cuda", non_blocking=True) for _, v in flatten(e.sample) if v is not None]
        host.update_priorities(e.sampling_indices, new_priorities[r])
        return leaves

    out = dict(max_size=args.max_size, Tb=args.tb, B=args.batch, rounds=args.rounds)
    for name, fn in (("device_round_ms", device_round), ("host_round_ms", host_round)):
        for r in range(3):
            keep = fn(args.rounds + r)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for r in range(args.rounds):
            keep = fn(r)
        torch.cuda.synchronize()
        out[name] = 1e3 * (time.perf_counter() - t0) / args.rounds
        del keep

    # the frame leaf's gather alone
    frames = next(s for k, s in zip(dev._keys, dev._store) if k == "obs.obs")
    row = frames["pad"]
    idx = dev.get().sampling_indices
    dst = torch.empty((args.tb, args.batch, row), dtype=torch.uint8, device="cuda")
    call = lambda: hip.replay_gather(frames["bytes"].data_ptr(), args.max_size, idx, args.batch, args.tb, row, dst.data_ptr())
    for _ in range(5):
        call()
    windows = []
    for _ in range(7):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(20):
            call()
        b.record()
        torch.cuda.synchronize()
        windows.append(1e3 * a.elapsed_time(b) / 20)
    nbytes = 2 * args.tb * args.batch * row
    out.update(gather_us=float(np.median(windows)), gather_bytes=nbytes, gather_floor_us=1e6 * nbytes / HBM_BYTES_PER_S,
               gather_us_windows=[round(w, 2) for w in windows])
    out["gather_share_of_floor"] = out["gather_floor_us"] / out["gather_us"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
