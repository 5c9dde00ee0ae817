"""Noisy networks (Fortunato et al., "Noisy Networks for Exploration"):
linear layers with factorised Gaussian parameter noise, and the dueling
C51 head RAINBOW uses them in.

The layer's forward and gradients run through
:func:`machin_amd.ops.noisy_linear` (fused gfx950 kernels on ROCm) and
its noise through :func:`machin_amd.ops.factorised_noise_`: one launch
per layer fills ``eps_in`` and ``eps_out`` together.
"""
import itertools
import math
import weakref
from typing import List, Optional

import torch as t
import torch.nn as nn
import torch.nn.functional as F

from ... import ops

_default_seeds = itertools.count(1)
# reset_noise's per-module [seed, counter], keyed by the module OBJECT:
# a copy.deepcopy of a net is a new object without an entry, so it never
# continues the stream of the net it was copied from
_noise_state = weakref.WeakKeyDictionary()
_SEED_MASK = (1 << 63) - 1
# reset_noise packs (call counter, layer stream id) into the Philox
# offset: the low bits are the layer's position in the net
_STREAM_BITS = 16


class NoisyLinear(nn.Module):
    """``y = x (mu_w + sigma_w * eps_out eps_in^T)^T + mu_b + sigma_b *
    eps_out`` with ``eps = f(z)``, ``f(z) = sign(z) sqrt(|z|)``.

    Parameters are ``weight_mu``, ``weight_sigma`` ``[O, I]`` and
    ``bias_mu``, ``bias_sigma`` ``[O]``, initialised as in the paper:
    ``mu ~ U(-1/sqrt(I), 1/sqrt(I))``, ``sigma = sigma0 / sqrt(I)``.

    The noise lives in one NON-persistent buffer ``eps`` of ``I + O``
    elements (``eps_in`` and ``eps_out`` are views of it): it follows
    ``.to(device)`` but stays out of ``state_dict``, so ``hard_update``
    and ``soft_update`` move parameters only and a target net keeps its
    own noise. New noise comes from :func:`reset_noise`; with
    ``noise_enabled = False`` (see :func:`noise_enabled`) the layer is
    ``F.linear(x, weight_mu, bias_mu)``.
    """

    def __init__(self, in_features: int, out_features: int,
                 sigma0: float = 0.5):
        super().__init__()
        if in_features < 1 or out_features < 1:
            raise ValueError("in_features and out_features must be >= 1")
        self.in_features = int(in_features)
        self.out_features = int(out_features)
        self.sigma0 = float(sigma0)
        self.noise_enabled = True
        self.weight_mu = nn.Parameter(t.empty(out_features, in_features))
        self.weight_sigma = nn.Parameter(t.empty(out_features, in_features))
        self.bias_mu = nn.Parameter(t.empty(out_features))
        self.bias_sigma = nn.Parameter(t.empty(out_features))
        self.register_buffer(
            "eps", t.zeros(in_features + out_features), persistent=False
        )
        self.reset_parameters()
        # a first draw, so that a fresh layer is noisy before the first
        # reset_noise; seeded from torch's global generator
        ops.factorised_noise_(
            self.eps, int(t.randint(0, 2 ** 62, (1,)).item()), 0
        )

    def reset_parameters(self):
        bound = 1.0 / math.sqrt(self.in_features)
        with t.no_grad():
            self.weight_mu.uniform_(-bound, bound)
            self.bias_mu.uniform_(-bound, bound)
            self.weight_sigma.fill_(self.sigma0 * bound)
            self.bias_sigma.fill_(self.sigma0 * bound)

    @property
    def eps_in(self) -> t.Tensor:
        return self.eps[: self.in_features]

    @property
    def eps_out(self) -> t.Tensor:
        return self.eps[self.in_features:]

    def forward(self, x: t.Tensor) -> t.Tensor:
        if not self.noise_enabled:
            return F.linear(x, self.weight_mu, self.bias_mu)
        return ops.noisy_linear(
            x, self.weight_mu, self.weight_sigma, self.bias_mu,
            self.bias_sigma, self.eps_in, self.eps_out,
        )

    def extra_repr(self) -> str:
        return (f"in_features={self.in_features}, "
                f"out_features={self.out_features}, sigma0={self.sigma0}")


def noisy_layers(module: nn.Module) -> List[NoisyLinear]:
    """The NoisyLinear layers of ``module`` in registration order."""
    return [m for m in module.modules() if isinstance(m, NoisyLinear)]


def reset_noise(module: nn.Module, seed: Optional[int] = None) -> None:
    """Draw new noise for every NoisyLinear of ``module``: one
    :func:`machin_amd.ops.factorised_noise_` call (one launch) per
    layer and no host-device synchronisation.

    Every module object has a seed and a call counter of its own, kept
    outside the module, so neither ``state_dict`` nor ``copy.deepcopy``
    carries them. The k-th layer in registration order is stream ``k``;
    the Philox offset of a draw is ``counter * 2^16 + k``, so equal-sized
    layers of one net and consecutive calls get different noise. Passing
    ``seed`` sets the module's seed and restarts its counter, which
    makes the draw reproducible; without one the module keeps its seed,
    by default one derived from ``torch.initial_seed()`` and the number
    of modules seeded before it in this process. A deep copy of a net
    (a target net made from the online net, before or after the online
    net's first draw) starts with such a default seed of its own, so the
    two draw independently.
    """
    state = _noise_state.get(module)
    if seed is not None:
        state = _noise_state[module] = [int(seed) & _SEED_MASK, 0]
    elif state is None:
        state = _noise_state[module] = [(
            t.initial_seed() * 0x9E3779B97F4A7C15
            + next(_default_seeds) * 0xD2511F53
        ) & _SEED_MASK, 0]
    noise_seed, counter = state
    state[1] = counter + 1
    layers = noisy_layers(module)
    if len(layers) >= 1 << _STREAM_BITS:
        raise ValueError("too many NoisyLinear layers in one module")
    for k, layer in enumerate(layers):
        ops.factorised_noise_(
            layer.eps, noise_seed,
            ((counter << _STREAM_BITS) | k) & _SEED_MASK,
        )


class noise_enabled:
    """Switch the noise of every NoisyLinear of ``module`` on or off.

    A setter, ``noise_enabled(net, False)``, and a context manager that
    puts every layer's previous setting back::

        with noise_enabled(net, False):
            greedy = net(state)
    """

    def __init__(self, module: nn.Module, flag: bool):
        self._layers = noisy_layers(module)
        self._previous = [layer.noise_enabled for layer in self._layers]
        for layer in self._layers:
            layer.noise_enabled = bool(flag)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for layer, flag in zip(self._layers, self._previous):
            layer.noise_enabled = flag
        return False


class NoisyDuelingC51Head(nn.Module):
    """Dueling distributional head of Rainbow on noisy layers: a value
    stream ``[B, 1, N]`` and an advantage stream ``[B, A, N]``, each
    ``NoisyLinear -> ReLU -> NoisyLinear``, combined per atom into the
    LOGITS ``v + a - a.mean(dim=1, keepdim=True)`` ``[B, A, N]`` (fp32).
    Use it with ``RAINBOW(fused_loss=True, dist_from_logits=True,
    noisy_nets=True)``."""

    def __init__(self, feature_dim: int, action_num: int, atom_num: int,
                 hidden: int = 512, sigma0: float = 0.5):
        super().__init__()
        self.action_num, self.atom_num = int(action_num), int(atom_num)
        self.value_hidden = NoisyLinear(feature_dim, hidden, sigma0)
        self.value_out = NoisyLinear(hidden, atom_num, sigma0)
        self.advantage_hidden = NoisyLinear(feature_dim, hidden, sigma0)
        self.advantage_out = NoisyLinear(
            hidden, action_num * atom_num, sigma0
        )

    def forward(self, feature: t.Tensor) -> t.Tensor:
        v = self.value_out(F.relu(self.value_hidden(feature)))
        a = self.advantage_out(F.relu(self.advantage_hidden(feature)))
        v = v.float().view(-1, 1, self.atom_num)
        a = a.float().view(-1, self.action_num, self.atom_num)
        return v + a - a.mean(dim=1, keepdim=True)
