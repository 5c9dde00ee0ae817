"""RAINBOW: distributional C51 + prioritized replay + n-step returns.

Parity target: reference ``machin/frame/algorithms/rainbow.py``
(:179-301): n-step reward folding at ``store_episode`` time
(machin_amd.ops.nstep_returns), categorical projection of
``r + gamma^n * z`` onto the fixed support (gfx950 kernel
machin_amd.ops.categorical_projection on GPU), cross-entropy loss
weighted by IS weights, abs-TD-style priority write-back.

Model contract: ``qnet(state) -> [batch, action_num, atom_num]``
distribution (softmaxed over atoms), or the logits of it with
``dist_from_logits=True``.

``fused_loss=True`` computes everything between the three network
forwards and ``backward()`` with :func:`machin_amd.ops.c51_loss` (one
gfx950 kernel each way on ROCm) in place of the eager chain; same
values. It is required by ``dist_from_logits`` and by
``exact_nstep_bootstrap=True``, which bootstraps every sample with
``discount ** m`` for the ``m`` steps its n-step window really covers
(needs a replay buffer that returns ``m`` as the ``n_step`` attribute,
i.e. ``DeviceFrameStackBuffer(n_step > 1)``).

``noisy_nets=True`` explores with noisy networks instead of epsilon:
both nets must contain :class:`machin_amd.model.nets.NoisyLinear`
layers (e.g. a ``NoisyDuelingC51Head``). ``update`` draws new,
independent noise for the online and the target net before the
forwards, ``act_discrete_with_noise`` draws new noise for the online
net and returns the argmax of every row (no epsilon, no host RNG read),
and ``act_discrete`` runs with the noise switched off.
"""
from typing import Any, Dict, List, Union

import numpy as np
import torch as t
import torch.nn as nn

from ... import ops
from ...model.nets.noisy import noise_enabled, noisy_layers, reset_noise
from ..buffers.prioritized_buffer import PrioritizedBuffer
from ..transition import Transition
from .dqn_per import DQNPer
from .utils import hard_update, safe_call, safe_return, soft_update


class RAINBOW(DQNPer):
    def __init__(
        self,
        qnet,
        qnet_target,
        optimizer,
        value_min: float,
        value_max: float,
        *_,
        criterion=None,
        reward_future_steps: int = 3,
        replay_size: int = 500000,
        replay_device: Union[str, t.device] = "cpu",
        replay_buffer=None,
        fused_loss: bool = False,
        dist_from_logits: bool = False,
        exact_nstep_bootstrap: bool = False,
        noisy_nets: bool = False,
        **kwargs,
    ):
        if dist_from_logits and not fused_loss:
            raise ValueError("dist_from_logits=True requires fused_loss=True.")
        if exact_nstep_bootstrap and not fused_loss:
            raise ValueError(
                "exact_nstep_bootstrap=True requires fused_loss=True."
            )
        super().__init__(
            qnet,
            qnet_target,
            optimizer,
            criterion or nn.MSELoss(reduction="none"),
            replay_size=replay_size,
            replay_device=replay_device,
            replay_buffer=replay_buffer,
            **kwargs,
        )
        self.v_min = float(value_min)
        self.v_max = float(value_max)
        self.reward_future_steps = reward_future_steps
        self.fused_loss = bool(fused_loss)
        self.dist_from_logits = bool(dist_from_logits)
        self.exact_nstep_bootstrap = bool(exact_nstep_bootstrap)
        self.noisy_nets = bool(noisy_nets)
        if self.noisy_nets:
            for name, net in (("qnet", self.qnet),
                              ("qnet_target", self.qnet_target)):
                if not noisy_layers(net):
                    raise ValueError(
                        f"noisy_nets=True but {name} contains no "
                        "NoisyLinear layer."
                    )
            # independent streams for the two nets, reproducible under
            # torch.manual_seed
            seed = int(t.randint(0, 2 ** 62, (1,)).item())
            reset_noise(self.qnet, seed=seed)
            reset_noise(self.qnet_target, seed=seed + 1)

    # ------------------------------------------------------------------
    def _criticize(self, state: Dict[str, Any], use_target: bool = False,
                   **__):
        """Returns the distribution [B, A, N]."""
        net = self.qnet_target if use_target else self.qnet
        return safe_return(safe_call(net, state))

    def _q_values(self, dist: t.Tensor) -> t.Tensor:
        B, A, N = dist.shape
        if self.dist_from_logits:
            dist = t.softmax(dist.float(), dim=2)
        support = t.linspace(
            self.v_min, self.v_max, N, device=dist.device
        )
        return (dist * support.view(1, 1, N)).sum(dim=2)

    def act_discrete(self, state, use_target=False, **__):
        if self.noisy_nets:
            net = self.qnet_target if use_target else self.qnet
            with noise_enabled(net, False):
                q = self._q_values(self._criticize(state, use_target))
            return t.argmax(q, dim=1).view(-1, 1)
        q = self._q_values(self._criticize(state, use_target))
        return t.argmax(q, dim=1).view(-1, 1)

    def act_discrete_with_noise(self, state, use_target=False,
                                decay_epsilon=True, **__):
        if self.noisy_nets:
            # exploration is the net's own noise: new noise, then the
            # greedy action of every row
            reset_noise(self.qnet_target if use_target else self.qnet)
            q = self._q_values(self._criticize(state, use_target))
            return t.argmax(q, dim=1).view(-1, 1)
        q = self._q_values(self._criticize(state, use_target))
        batch, n_actions = q.shape
        if t.rand(1).item() < self.epsilon:
            result = t.randint(0, n_actions, (batch, 1))
        else:
            result = t.argmax(q, dim=1).view(-1, 1)
        if decay_epsilon:
            self.epsilon *= self.epsilon_decay
        return result

    # ------------------------------------------------------------------
    def store_episode(self, episode: List[Union[Transition, Dict]]):
        """Fold the next ``reward_future_steps`` rewards into each
        transition before storing (n-step returns).

        A replay buffer that folds n-step returns itself when sampling
        (``replay_buffer.n_step > 1``, see
        :class:`..buffers.frame_stack_buffer.DeviceFrameStackBuffer`)
        gets the raw 1-step episode instead; its ``n_step`` and
        ``discount`` must equal this algorithm's
        ``reward_future_steps`` and ``discount``. Sampled rows are then
        what the host fold stores, and ``update`` bootstraps every
        sample with ``discount ** reward_future_steps`` on both paths,
        windows cut short by the episode's end included. The buffer
        also returns the per-sample step count ``m`` as the custom
        attribute ``n_step``; with ``exact_nstep_bootstrap=True``
        (needs ``fused_loss=True``) ``update`` bootstraps with
        ``discount ** m`` instead, which differs for windows cut short
        by a non-terminal episode end (a time limit).
        """
        buffer_n = getattr(self.replay_buffer, "n_step", 1)
        if buffer_n > 1:
            buffer_discount = self.replay_buffer.discount
            if buffer_n != self.reward_future_steps \
                    or abs(buffer_discount - self.discount) >= 1e-12:
                raise ValueError(
                    f"Replay buffer folds n-step returns with n_step="
                    f"{buffer_n}, discount={buffer_discount}, but the "
                    f"algorithm has reward_future_steps="
                    f"{self.reward_future_steps}, discount="
                    f"{self.discount}."
                )
            self.replay_buffer.store_episode(
                episode,
                required_attrs=("state", "action", "next_state", "reward",
                                "terminal"),
            )
            return
        episode = [
            Transition(**tr) if isinstance(tr, dict) else tr for tr in episode
        ]
        n = self.reward_future_steps
        if n > 1:
            T = len(episode)
            rewards = t.tensor(
                [float(tr.reward) if not t.is_tensor(tr.reward)
                 else float(tr.reward.reshape(-1)[0]) for tr in episode]
            )
            terminals = t.tensor(
                [float(tr.terminal) if not t.is_tensor(tr.terminal)
                 else float(tr.terminal.reshape(-1)[0]) for tr in episode]
            )
            nstep = ops.nstep_returns(rewards, terminals, self.discount, n)
            # single host copy for the whole episode (no per-element
            # .item() synchronization)
            nstep_list = nstep.tolist()
            term_list = terminals.tolist()
            new_episode = []
            for i, tr in enumerate(episode):
                d = {k: getattr(tr, k) for k in tr.keys()}
                d["reward"] = float(nstep_list[i])
                # bootstrap state is s_{i+n} (or the episode end)
                j = min(i + n - 1, T - 1)
                d["next_state"] = {
                    k: v for k, v in episode[j].next_state.items()
                }
                d["terminal"] = bool(max(term_list[i : j + 1]) > 0.5)
                new_episode.append(Transition(**d))
            episode = new_episode
        self.replay_buffer.store_episode(
            episode,
            required_attrs=("state", "action", "next_state", "reward", "terminal"),
        )

    # ------------------------------------------------------------------
    def _bootstrap_discount(self, others, device):
        """Discount of the bootstrap term for the fused loss: the scalar
        ``discount ** reward_future_steps``, or with
        ``exact_nstep_bootstrap`` the f32 ``[B]`` tensor
        ``discount ** m`` from the sampled ``n_step`` attribute."""
        if not self.exact_nstep_bootstrap:
            return self.discount ** self.reward_future_steps
        steps = others.get("n_step") if isinstance(others, dict) else None
        if not t.is_tensor(steps):
            raise ValueError(
                "exact_nstep_bootstrap=True needs the per-sample step "
                "count as the sampled attribute 'n_step'; a "
                "DeviceFrameStackBuffer(n_step > 1) provides it, "
                f"{type(self.replay_buffer).__name__} did not."
            )
        steps = steps.to(device=device, dtype=t.float32).view(-1)
        return t.pow(float(self.discount), steps)

    def update(self, update_value=True, update_target=True,
               concatenate_samples=True, **__):
        (
            batch_size,
            (state, action, reward, next_state, terminal, others),
            index,
            is_weight,
        ) = self.replay_buffer.sample_batch(
            self.batch_size,
            concatenate_samples,
            sample_attrs=["state", "action", "reward", "next_state", "terminal", "*"],
        )
        if batch_size == 0:
            return 0.0
        self.qnet.train()
        if self.noisy_nets:
            reset_noise(self.qnet)
            reset_noise(self.qnet_target)

        dist = self._criticize(state)  # [B, A, N]
        B, A, N = dist.shape
        device = dist.device
        action_index = action["action"].to(device=device, dtype=t.long).view(B)

        if self.fused_loss:
            # action selection, gather, projection and cross entropy in
            # one op (one kernel each way on ROCm)
            with t.no_grad():
                online_next = self._criticize(next_state)
                target_next = self._criticize(next_state, use_target=True)
            per_sample, _, _ = ops.c51_loss(
                dist, action_index, online_next, target_next,
                reward.to(device), terminal.to(device),
                self._bootstrap_discount(others, device),
                self.v_min, self.v_max,
                from_logits=self.dist_from_logits,
            )
        else:
            with t.no_grad():
                # double-DQN action selection with the online net
                online_next = self._criticize(next_state)
                next_q = self._q_values(online_next)
                best = next_q.argmax(dim=1)  # [B]
                target_next = self._criticize(next_state, use_target=True)
                next_dist = target_next[
                    t.arange(B, device=device), best
                ]  # [B,N]
                reward = reward.to(device).float().view(B)
                terminal = terminal.to(device).float().view(B)
                gamma_n = self.discount ** self.reward_future_steps
                proj = ops.categorical_projection(
                    next_dist, reward, terminal, gamma_n, self.v_min,
                    self.v_max
                )

            pred = dist[t.arange(B, device=device), action_index]  # [B,N]
            log_pred = t.log(pred.clamp_min(1e-8))
            per_sample = -(proj * log_pred).sum(dim=1)  # cross entropy
        weights = t.as_tensor(
            is_weight, dtype=per_sample.dtype, device=device
        ).view(B)
        loss = (per_sample * weights).mean()

        if getattr(self.replay_buffer, "accepts_tensor_priorities", False):
            self.replay_buffer.update_priority(per_sample.detach(), index)
        else:
            self.replay_buffer.update_priority(
                per_sample.detach().cpu().numpy().astype(np.float64), index
            )

        if self.visualize:
            self.visualize_model(loss, "qnet", self.visualize_dir)
        if update_value:
            self.qnet_optim.zero_grad(set_to_none=True)
            self._backward(loss)
            nn.utils.clip_grad_norm_(self.qnet.parameters(), self.grad_max)
            self.qnet_optim.step()
        if update_target:
            if self.update_rate is not None:
                soft_update(self.qnet_target, self.qnet, self.update_rate)
            else:
                self._update_counter += 1
                if self._update_counter % self.update_steps == 0:
                    hard_update(self.qnet_target, self.qnet)
        return float(loss.detach().item())

    # ------------------------------------------------------------------
    @classmethod
    def generate_config(cls, config):
        from .dqn import DQN

        config = DQN.generate_config(config)
        config["frame"] = "RAINBOW"
        fc = config["frame_config"]
        fc["frame"] = "RAINBOW"
        fc.pop("mode", None)
        fc.setdefault("value_min", -10.0)
        fc.setdefault("value_max", 10.0)
        fc.setdefault("reward_future_steps", 3)
        fc.setdefault("noisy_nets", False)
        return config

    @classmethod
    def init_from_config(cls, config, model_device="cpu"):
        from ...utils.conf import Config
        from .utils import (
            assert_and_get_valid_criterion,
            assert_and_get_valid_models,
            assert_and_get_valid_optimizer,
        )

        data = config.data if isinstance(config, Config) else dict(config)
        fc = data["frame_config"]
        model_cls = assert_and_get_valid_models(fc["models"])
        models = [
            m(*args, **kwargs).to(model_device)
            for m, args, kwargs in zip(
                model_cls, fc.get("model_args", ((), ())),
                fc.get("model_kwargs", ({}, {})),
            )
        ]
        optimizer = assert_and_get_valid_optimizer(fc["optimizer"])
        criterion = assert_and_get_valid_criterion(fc["criterion"])(
            *fc.get("criterion_args", ()), **fc.get("criterion_kwargs", {})
        )
        return cls(
            models[0], models[1], optimizer,
            fc["value_min"], fc["value_max"],
            criterion=criterion,
            **{
                k: v
                for k, v in fc.items()
                if k
                not in (
                    "frame", "models", "model_args", "model_kwargs",
                    "optimizer", "criterion", "criterion_args",
                    "criterion_kwargs", "lr_scheduler", "value_min",
                    "value_max", "mode",
                )
            },
        )
