"""Phasic Policy Gradient on Normal action heads, off the device: the float32 CPU restatement (tests/ppg_gauss_ref.py) against the
vectors the reference produced (tests/golden/ppg_gauss.npz, gen_ppg_gauss.py), at the bars tests/test_gpu_ppg.py holds the device
path to; and the built library's side of the feature (the exported kernel entry, ABI 21)."""
import ctypes

import numpy as np
import pytest
import torch

from oracle.net import OracleActorCritic
from ppg_cases import entry_arrays, params_of
from ppg_gauss_cases import PPG_GAUSS_CASES
from ppg_gauss_ref import GaussPPGAux
from srl_amd import hip
from srl_amd.runtime import synthetic


@pytest.mark.parametrize("tag", list(PPG_GAUSS_CASES))
def test_float32_restatement_reproduces_reference_golden(tag, golden):
    g = golden("ppg_gauss.npz")
    pargs, targs, skw = PPG_GAUSS_CASES[tag]
    net = OracleActorCritic(**pargs)
    net.load_state_dict(params_of(g, tag, "init"))
    aux = GaussPPGAux(net, beta_clone=targs.get("beta_clone", 1), aux_value_head_weight=targs.get("aux_value_head_weight", 1),
                      max_grad_norm=targs.get("max_grad_norm"), popart=targs.get("popart", False),
                      ppg_optimizer_config=targs.get("ppg_optimizer_config", {}))
    e = entry_arrays(synthetic.make_sample_arrays(seed=300, **skw), skw["T"], g, tag)
    aux.enter(e)
    assert np.abs(aux.mean_old.numpy() - g[f"{tag}_p2_loc"]).max() <= 1e-5
    assert np.abs(aux.log_std_old.exp().numpy() - g[f"{tag}_p2_scale"]).max() <= 1e-5
    pert = params_of(g, tag, "pert")
    for k, p in net.params.items():
        p.data.copy_(torch.from_numpy(pert[k]).to(p.dtype))
    names = list(g["term_names"])
    for ep in range(targs["ppg_epochs"]):
        o = aux.epoch(e)
        ref = dict(zip(names, g[f"{tag}_epoch{ep}_terms"]))
        for k in ("auxiliary_value_loss", "value_head_loss", "policy_distance"):
            assert abs(o[k] - ref[k]) <= 1e-5 * max(abs(ref[k]), 1e-2), (ep, k, o[k], ref[k])
        assert (ref["grad_norm"] >= 0) == (targs.get("max_grad_norm") is not None)
        if ref["grad_norm"] >= 0:
            assert abs(o["grad_norm"] - ref["grad_norm"]) <= 2e-5 * max(ref["grad_norm"], 1e-2), (ep, o["grad_norm"], ref["grad_norm"])
    sd = net.state_dict()
    for k, v in params_of(g, tag, "final").items():
        assert np.abs(sd[k].numpy() - v).max() <= 2e-5, (k, np.abs(sd[k].numpy() - v).max())
    if pargs["std_type"] == "fixed":
        assert np.array_equal(sd["log_std"].numpy(), pert["log_std"])


def test_library_exports_gaussian_aux_loss_at_abi_22():
    lib = ctypes.CDLL(hip.library_path())
    assert hasattr(lib, "srl_ppg_aux_loss_gaussian_fwd_bwd")
    assert "srl_ppg_aux_loss_gaussian_fwd_bwd" in hip.EXPORTED_SYMBOLS
    lib.srl_abi_version.restype = ctypes.c_int
    # (exported since ABI 22; 23 took the 2-D copies of the channels-last volume entry points away, nothing else)
    assert lib.srl_abi_version() == 23 and hip.ABI_VERSION == 23
