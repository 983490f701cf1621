"""``q-learning``: the deep Q-learning trainer on the HIP kernels.

Mirror of ``DeepQLearning`` (reference ``legacy/algorithm/q_learning/deep_q_learning.py:21-241``): the same constructor keywords and
defaults, the same statistics, ``TrainerStepResult.priorities`` for a prioritised replay buffer, checkpoints that carry both
networks and the optimiser.  One step is

    policy.analyze (both networks' forward passes; the recurrent agent's burn-in pass in front of them) -> srl_dqn_td_fwd_bwd (gathers, transforms, n-step return, loss, gradient
    with respect to the head outputs, priorities, statistics: csrc/dqn.hip) -> net.backward -> global-norm clip folded into the
    optimiser step (FlatOptimizer) -> soft target update every step, or a hard one by ``hard_update_interval`` -> inc_version

and the host waits for the device once, at the end, for the statistics and the priorities.  ``step(sample,
device_priorities=True)`` serves a replay buffer resident in HBM (runtime/replay.py): ``TrainerStepResult.priorities`` stays a device
tensor, ``sampling_weight`` and ``policy_state.epsilon`` may be device tensors, and the means the statistics report of the three
(``srl_pairwise_means``: numpy's float32 mean, so both paths log the same numbers) travel in the block the step reads back anyway --
still one wait.  (``info`` statistics of a sample whose leaves are device tensors are read back on their own.)

DIFFERENCES: a sample is consumed by the call that receives it (the reference's GPU prefetcher hands ``step`` the PREVIOUS
call's sample and returns an empty result for the first one, :91-96).  ``use_popart=True`` (the reference's ``atari-dqn`` policy has
no ``denormalize_target_value`` either) and ``mixed_precision=True`` raise at construction; a process group is refused.
``burn_in_steps`` is handed to ``policy.analyze`` and cut off every other leaf, as in the reference; with the recurrent ``atari-dqn``
the burn-in rows run through the online network only, and the conv features of rows that are both burn-in and analysed rows are
computed twice (not shared between the passes).
"""
import numpy as np
import torch
import torch.distributed as dist

from srl_amd import hip
from srl_amd.algorithm.actor_critic import to_device_leaf
from srl_amd.algorithm.optim import FlatOptimizer
from srl_amd.api.trainer import PytorchTrainer, TrainerStepResult, register
from srl_amd.namedarray import recursive_apply


class DeepQLearning(PytorchTrainer):

    def __init__(self, policy, **kwargs):
        super().__init__(policy)
        g = kwargs.get
        self.gamma = g("gamma", 0.99)
        self.bootstrap_steps = g("bootstrap_steps", 1)
        if self.bootstrap_steps <= 0:
            raise ValueError("bootstrap_steps of Q-Learning must be a positive integer!")
        self.burn_in_steps = g("burn_in_steps", 0)
        self.use_soft_update = g("use_soft_update", False)
        self.tau = g("tau", 0.005)
        self.hard_update_interval = g("hard_update_interval", 200)
        self.max_grad_norm = g("max_grad_norm", None)
        self.use_popart = g("use_popart", False)
        self.apply_scalar_transform = g("apply_scalar_transform", True)
        if self.use_popart and self.apply_scalar_transform:
            raise ValueError("use_popart and apply_scalar_transform cannot be True simultaneously!")
        if self.use_popart:
            raise NotImplementedError("q-learning: use_popart=True is not implemented (the atari-dqn policy has no PopArt head)")
        self.scalar_transform_eps = g("scalar_transform_eps", 1e-3)
        self.use_priority_weight = g("use_priority_weight", False)
        self.priority_interpolation_eta = g("priority_interpolation_eta", 0.9)
        self.gpu_prefetching = g("gpu_prefetching", True)  # accepted; the sample is consumed in the call that receives it
        self.mixed_precision = g("mixed_precision", False)
        if self.mixed_precision:
            raise NotImplementedError("q-learning: mixed_precision=True is not implemented (the scalar transforms need float32)")
        if not hasattr(policy, "backward_dqn"):
            raise NotImplementedError(f"q-learning: {type(policy).__name__} has no analyze(target='dqn') on the HIP path")
        self.optimizer = FlatOptimizer(policy.net, g("optimizer", "adam"),
                                       g("optimizer_config", dict(lr=5e-4, eps=1e-5, weight_decay=0.)), "optimizer_config")
        value_loss = g("value_loss", "mse")
        if value_loss not in hip.VALUE_LOSS_KINDS:
            raise AssertionError(f"Value loss name {value_loss} does not match any implemented loss functions "
                                 f"({list(hip.VALUE_LOSS_KINDS)})")
        vcfg = g("value_loss_config", {})
        self._hp = hip.DqnHparams(gamma=float(self.gamma), scalar_transform_eps=float(self.scalar_transform_eps),
                                  priority_interpolation_eta=float(self.priority_interpolation_eta),
                                  huber_delta=float(vcfg.get("delta", vcfg.get("beta", 1.0))), n=int(self.bootstrap_steps),
                                  apply_scalar_transform=int(bool(self.apply_scalar_transform)),
                                  double_q=int(bool(getattr(policy, "use_double_q", True))),
                                  value_loss=hip.VALUE_LOSS_KINDS[value_loss])
        self.last_hard_update_step = 0
        self.hard_update_count = 0
        self.steps = 0
        self.frames = 0
        self.total_timesteps = 0

    # ------------------------------------------------------------------ checkpoints (:27-35)
    def get_checkpoint(self):
        checkpoint = self.policy.get_checkpoint()
        checkpoint.update({"optimizer_state_dict": self.optimizer.state_dict()})
        return checkpoint

    def load_checkpoint(self, checkpoint, **kwargs):
        if "optimizer_state_dict" in checkpoint.keys():
            self.optimizer.load_state_dict(checkpoint["optimizer_state_dict"], "optimizer_state_dict")
        self.policy.load_checkpoint(checkpoint)

    def distributed(self, rank=None, world_size=None, init_method=None, **kwargs):
        raise NotImplementedError("q-learning: data-parallel training is not implemented")

    # ------------------------------------------------------------------ the step (:90-238)
    def step(self, sample, device_priorities=False):
        hip.require_gpu()
        if dist.is_initialized():
            raise NotImplementedError("q-learning: data-parallel training is not implemented (a process group is initialised)")
        policy, net = self.policy, self.policy.net
        dev = policy.device
        Tb = sample.on_reset.shape[0]
        burn, n_boot = self.burn_in_steps, self.bootstrap_steps
        sample_steps = Tb - burn - n_boot
        if sample_steps <= 0:
            raise RuntimeError("Sample length should be larger than bootstrap_steps for Q-learning!")

        net.zero_grad()
        out = policy.analyze(sample, target="dqn", burn_in_steps=burn)
        T, B, n = out.T, out.B, out.T * out.B
        leaf = lambda x, kind: to_device_leaf(x, dev, kind)[burn:].reshape(n)
        reward, done, truncated = leaf(sample.reward, "real"), leaf(sample.done, "flag"), leaf(sample.truncated, "flag")
        host_weight = sample.metadata.get("sampling_weight")
        weight = None
        if self.use_priority_weight and host_weight is not None:
            weight = to_device_leaf(host_weight, dev, "real").reshape(B)

        ws = net.ws
        d_adv = ws.get("dqn.d_adv", out.adv.numel())[:out.adv.numel()].view_as(out.adv)
        d_v = ws.get("dqn.d_v", n)[:n]
        priorities = ws.get("dqn.priorities", B)[:B]
        # one block for everything the host reads back: the TD terms, then the gradient norm (float32 in a float64 slot), then
        # (device_priorities) the means of the new priorities, the sampling weights and epsilon
        n_back = hip.DQ_COUNT + 1 + (3 if device_priorities else 0)
        back = ws.get("dqn.terms", hip.DQ_COUNT + 4, torch.float64)[:n_back]
        terms, gn = back[:hip.DQ_COUNT], back[hip.DQ_COUNT:hip.DQ_COUNT + 1].view(torch.float32)[:1]
        hip.dqn_td_fwd_bwd(out.adv, out.value.reshape(n), out.target_adv, out.target_value.reshape(n), out.action, reward, done,
                           truncated, weight, T, B, self._hp, d_adv, d_v, terms, priorities)
        policy.backward_dqn(d_adv, d_v)

        # clip_grad_norm_ (max_grad_norm) or the plain norm (:164-167), folded into the optimiser's launch
        sumsq = ws.get("dqn.sumsq", 1, torch.float64)[:1]
        hip.grad_sumsq(net.grad, sumsq)
        self.optimizer.step(net, ahead=0, grad_scale=1.0, sumsq=sumsq, grad_norm_out=gn,
                            max_norm=-1.0 if self.max_grad_norm is None else float(self.max_grad_norm))
        self.optimizer.steps += 1
        net.params_changed()

        # update target network (:196-204)
        if self.use_soft_update:
            policy.soft_target_update(self.tau)
        elif (self.steps - self.last_hard_update_step) / self.hard_update_interval >= 1.:
            policy.hard_target_update()
            self.last_hard_update_step = self.steps
            self.hard_update_count += 1
        self.steps += 1

        eps = getattr(sample.policy_state, "epsilon", None) if sample.policy_state is not None else None
        if device_priorities:
            on_device = lambda x: x.to(dev, torch.float32).contiguous() if isinstance(x, torch.Tensor) and x.is_cuda else None
            hip.pairwise_means([priorities, on_device(host_weight), on_device(eps)], back[hip.DQ_COUNT + 1:])
        host = back.cpu()  # the step's first wait for the device
        t = host[:hip.DQ_COUNT].numpy()
        grad_norm = float(host[hip.DQ_COUNT:hip.DQ_COUNT + 1].view(torch.float32)[0])
        cnt = t[hip.DQ_MASK]
        self.total_timesteps += cnt
        mean = lambda slot: float(t[slot] / cnt) if cnt > 0 else float("nan")
        if device_priorities:
            new_priorities = priorities.clone()  # the workspace's next step overwrites it
            means = host[hip.DQ_COUNT + 1:].numpy()
            of = lambda x, k: float(means[k]) if isinstance(x, torch.Tensor) and x.is_cuda else float(np.asarray(x).mean())
            mean_priority = float(means[0])
            mean_weight = of(host_weight, 1) if host_weight is not None else 0.0
            mean_eps = of(eps, 2) if eps is not None else 0.0
        else:
            new_priorities = priorities.cpu().numpy().copy()
            mean_priority = float(new_priorities.mean())
            to_host = lambda x: x.cpu() if isinstance(x, torch.Tensor) else x
            mean_weight = float(np.asarray(to_host(host_weight)).mean()) if host_weight is not None else 0.0
            mean_eps = float(np.asarray(eps.cpu() if isinstance(eps, torch.Tensor) else eps).mean()) if eps is not None else 0.0
        stats = dict(value_loss=mean(hip.DQ_VLOSS), grad_norm=grad_norm, train_q_tot=mean(hip.DQ_QINV),
                     target_q_tot=mean(hip.DQ_YINV), normalized_train_q_tot=mean(hip.DQ_Q),
                     normalized_target_q_tot=mean(hip.DQ_Y), mean_td_err=mean(hip.DQ_TD), max_td_err=float(t[hip.DQ_TDMAX]),
                     new_priorities=mean_priority, priority_weight=mean_weight, epsilon=mean_eps,
                     frames=int(self.frames), hard_update_count=self.hard_update_count,
                     total_timesteps=float(self.total_timesteps))

        lo, hi = burn, Tb - n_boot
        self.frames += int(np.prod(sample.on_reset[lo:hi].shape))
        policy.inc_version()

        if sample.info_mask is not None and sample.info is not None:
            im = sample.info_mask[lo:hi]
            im = im.cpu().numpy() if isinstance(im, torch.Tensor) else np.asarray(im)
            elapsed = im.sum()
            if elapsed > 0:
                host_info = recursive_apply(sample.info[lo:hi],
                                            lambda x: x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x))
                info = recursive_apply(host_info * im, lambda x: x.sum()) / elapsed
                stats.update({k: float(v) for k, v in info.items()})
        return TrainerStepResult(stats=stats, step=self.steps, priorities=new_priorities)


register("q-learning", DeepQLearning)
