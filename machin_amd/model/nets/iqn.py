"""Implicit quantile networks (Dabney et al., "Implicit Quantile Networks
for Distributional Reinforcement Learning"): the cosine embedding of
sampled quantile fractions and the head built on it.

The embedding and its gradients run through
:func:`machin_amd.ops.iqn_embedding` (fused gfx950 kernels on ROCm, a
torch composition on the CPU).
"""
import math

import torch as t
import torch.nn as nn
import torch.nn.functional as F

from ... import ops
from .noisy import NoisyLinear


class CosineTauEmbedding(nn.Module):
    """``h[b, n, :] = feature[b] * ReLU(W cos(pi i tau[b, n])_{i < n_cos}
    + bias)``: ``forward(feature [B, D], taus [B, N]) -> [B, N, D]`` in
    ``feature``'s dtype. ``weight [feature_dim, n_cos]`` and ``bias`` are
    initialised like ``nn.Linear(n_cos, feature_dim)``."""

    def __init__(self, feature_dim: int, n_cos: int = 64):
        super().__init__()
        if feature_dim < 1 or not 1 <= n_cos <= ops.IQN_EMBEDDING_MAX_COS:
            raise ValueError(
                "need feature_dim >= 1 and n_cos in "
                f"[1, {ops.IQN_EMBEDDING_MAX_COS}]"
            )
        self.feature_dim, self.n_cos = int(feature_dim), int(n_cos)
        self.weight = nn.Parameter(t.empty(feature_dim, n_cos))
        self.bias = nn.Parameter(t.empty(feature_dim))
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        bound = 1.0 / math.sqrt(self.n_cos)
        nn.init.uniform_(self.bias, -bound, bound)

    def forward(self, feature: t.Tensor, taus: t.Tensor) -> t.Tensor:
        return ops.iqn_embedding(feature, taus, self.weight, self.bias)

    def extra_repr(self) -> str:
        return f"feature_dim={self.feature_dim}, n_cos={self.n_cos}"


class ImplicitQuantileHead(nn.Module):
    """IQN head: embedding, ``Linear(D, hidden)``, ReLU,
    ``Linear(hidden, action_num)``. ``forward(feature [B, D], taus
    [B, N]) -> [B, action_num, N]`` quantile values in fp32, the ``theta``
    layout of :func:`machin_amd.ops.quantile_huber_loss`. ``noisy=True``
    builds the two linear layers as :class:`NoisyLinear`, for
    ``noisy_nets=True`` algorithms."""

    def __init__(self, feature_dim: int, action_num: int, hidden: int = 512,
                 n_cos: int = 64, noisy: bool = False):
        super().__init__()
        linear = NoisyLinear if noisy else nn.Linear
        self.action_num = int(action_num)
        self.embedding = CosineTauEmbedding(feature_dim, n_cos)
        self.hidden = linear(feature_dim, hidden)
        self.out = linear(hidden, action_num)

    def forward(self, feature: t.Tensor, taus: t.Tensor) -> t.Tensor:
        h = self.embedding(feature, taus)
        q = self.out(F.relu(self.hidden(h)))
        return q.float().transpose(1, 2)
