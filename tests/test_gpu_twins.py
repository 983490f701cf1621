"""The executors of a multi-pipeline update (`HipNet.twin`) over one `ParamState`: what they derive from the parameters is
made once for all of them, nothing they accumulate is left open, and they add up to the single executor's gradients."""
import functools

import pytest
import torch

import srl_amd
from srl_amd import hip
from srl_amd.runtime import synthetic
from test_gpu_trainer import ATARI_TRAINER, CNN_POLICY, make_trainer

srl_amd.register_all()
pytestmark = pytest.mark.gpu

COUNTED = ("h2_weights", "conv2d_obs_fold_h2", "presplit")
# Launches per step, (h2_weights, conv2d_obs_fold_h2, presplit), measured with this test on the parent of the commit that
# introduced `ParamState` (8eb52ab), the same for 1, 2 and 4 pipelines.  Per parameter version `H2Cnn._prepare_weights` makes
# six h2_weights calls (conv2 and conv3 in two orientations each, the Linear in two); the fold is a launch of its own only at
# the top of an update (`H2Cnn.prepare`) -- in the first step the blocks do not exist yet there, and the first chunk's forward
# kernel folds on its way; nothing on this path pre-splits through `HipNet._presplit`.
PARENT_COUNTS = [(6, 0, 0), (6, 1, 0)]


@functools.lru_cache(maxsize=None)
def _samples():
    return [synthetic.make_sample_arrays(seed=11 + step, T=1, B=1024, obs_spec=synthetic.ATARI_OBS, action_dims=6, p_done=0.05)
            for step in range(2)]


@functools.lru_cache(maxsize=None)
def _run(pipelines):
    """Two updates of four 256-row chunks (256: the smallest chunk on the pre-split block, HipNet.H2_MIN_ROWS).  The second
    update of every run starts from the parameters the single-pipeline run had there, so that its gradients compare."""
    start2 = None if pipelines == 1 else _run(1)["flat"]
    counts, out = dict.fromkeys(COUNTED, 0), dict(counts=[], grads=[], open=[])
    with pytest.MonkeyPatch.context() as mp:
        for name in COUNTED:
            def counting(*a, _name=name, _fn=getattr(hip, name), **kw):
                counts[_name] += 1
                return _fn(*a, **kw)
            mp.setattr(hip, name, counting)
        trainer = make_trainer(CNN_POLICY, dict(ATARI_TRAINER, chunk_rows=256, pipelines=pipelines))
        net = trainer.policy.net
        for step, arrays in enumerate(_samples()):
            if step == 1:
                if start2 is not None:
                    net.flat.copy_(start2)
                    net.params_changed()
                out["flat"] = net.flat.detach().cpu().clone()
            before = dict(counts)
            trainer.step(synthetic.to_sample_batch({k: v.copy() for k, v in arrays.items()}))
            out["counts"].append(tuple(counts[k] - before[k] for k in COUNTED))
            out["grads"].append({k: v.clone() for k, v in net.flat_to_reference(net.grad.detach().cpu()).items()})
            execs = [net] + list(trainer._twin or [])
            out["open"].append([b.open for x in execs for b in x._h2_blocks.values() if b is not None])
        out["executors"] = len(execs)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("pipelines", [1, 2, 4])
def test_twins_share_derived_weights_and_sum_to_the_single_executor(pipelines):
    """(1) derived-weight launches per step: what this test counted on commit 8eb52ab, the parent of the one that introduced
    `ParamState` -- six h2_weights per step, no fold launch in the first step and one in the second, no presplit
    (PARENT_COUNTS) -- whatever the number of pipelines;
    (2) no pre-split block of any executor is left open behind an update; (3) every gradient tensor of both updates against
    the single pipeline's, which sums the same four chunks in another order: max |difference| <= 2e-5 max |g|, the bound of
    test_first_layer_accumulation_with_a_ragged_last_chunk."""
    run, ref = _run(pipelines), _run(1)
    print(f"pipelines={pipelines}: executors={run['executors']} launches per step {dict(zip(COUNTED, zip(*run['counts'])))}")
    assert run["executors"] == pipelines
    assert run["counts"] == PARENT_COUNTS, run["counts"]
    assert all(len(blocks) == pipelines and not any(blocks) for blocks in run["open"]), run["open"]
    for step, (got, want) in enumerate(zip(run["grads"], ref["grads"])):
        for k, g0 in want.items():
            err, scale = float((got[k] - g0).abs().max()), float(g0.abs().max())
            print(f"  step {step} {k}: max|d|={err:.3e} max|g|={scale:.3e}")
            assert err <= 2e-5 * max(scale, 1e-8), (step, k, err, scale)
