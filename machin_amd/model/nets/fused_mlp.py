"""A whole MLP, or an ensemble of independent MLPs of one shape, as one
module whose forward and gradients run through
:func:`machin_amd.ops.fused_mlp` (fused gfx950 kernels on ROCm, a torch
composition on the CPU).
"""
import math
from typing import Optional, Sequence

import torch as t
import torch.nn as nn

from ... import ops


class FusedMLP(nn.Module):
    """``Linear(sizes[0], sizes[1])``, ReLU, ..., ``Linear(sizes[-2],
    sizes[-1])`` with no activation after the last layer: ``forward(x
    [B, sizes[0]]) -> [B, sizes[-1]]``.

    With ``ensemble=E`` the module holds ``E`` independent networks
    (twin critics, sub-policies): ``forward`` takes ``[E, B, sizes[0]]``,
    or ``[B, sizes[0]]`` shared by all members, and returns ``[E, B,
    sizes[-1]]``.

    ``weights[l]`` is ``[sizes[l + 1], sizes[l]]`` and ``biases[l]``
    ``[sizes[l + 1]]`` (with a leading ``E`` in an ensemble), every
    member initialised like ``nn.Linear``, independently. The state-dict
    keys are ``weights.<l>`` and ``biases.<l>``, not those of an
    ``nn.Sequential`` of ``nn.Linear``; :meth:`load_linears` moves an
    existing net over.
    """

    def __init__(self, sizes: Sequence[int], ensemble: Optional[int] = None):
        super().__init__()
        sizes = tuple(int(s) for s in sizes)
        layers = len(sizes) - 1
        if not 2 <= layers <= ops.FUSED_MLP_MAX_LAYERS:
            raise ValueError(
                f"need 2 to {ops.FUSED_MLP_MAX_LAYERS} linear layers"
            )
        if not all(1 <= s <= ops.FUSED_MLP_MAX_WIDTH for s in sizes):
            raise ValueError(
                f"every width must be in [1, {ops.FUSED_MLP_MAX_WIDTH}]"
            )
        if ensemble is not None and ensemble < 1:
            raise ValueError("ensemble must be None or at least 1")
        self.sizes, self.ensemble = sizes, ensemble
        lead = () if ensemble is None else (int(ensemble),)
        self.weights = nn.ParameterList(
            nn.Parameter(t.empty(*lead, sizes[l + 1], sizes[l]))
            for l in range(layers)
        )
        self.biases = nn.ParameterList(
            nn.Parameter(t.empty(*lead, sizes[l + 1])) for l in range(layers)
        )
        self.reset_parameters()

    @t.no_grad()
    def reset_parameters(self):
        for w, b in zip(self.weights, self.biases):
            members = [(w, b)] if self.ensemble is None else zip(w, b)
            bound = 1.0 / math.sqrt(w.shape[-1])
            for wm, bm in members:
                nn.init.kaiming_uniform_(wm, a=math.sqrt(5))
                nn.init.uniform_(bm, -bound, bound)

    @t.no_grad()
    def load_linears(self, linears, member: int = 0):
        """Copy weights and biases from ``nn.Linear`` modules (other
        modules of the sequence, such as the ``nn.ReLU`` of
        ``mlp(sizes)``, are skipped) into this net or into one member."""
        linears = [m for m in linears if isinstance(m, nn.Linear)]
        if len(linears) != len(self.weights):
            raise ValueError(f"need {len(self.weights)} nn.Linear modules")
        for w, b, lin in zip(self.weights, self.biases, linears):
            if self.ensemble is not None:
                w, b = w[member], b[member]
            if lin.bias is None or lin.weight.shape != w.shape:
                raise ValueError("a layer's shape or bias does not match")
            w.copy_(lin.weight)
            b.copy_(lin.bias)
        return self

    def forward(self, x: t.Tensor) -> t.Tensor:
        return ops.fused_mlp(x, list(self.weights), list(self.biases))

    def extra_repr(self) -> str:
        return f"sizes={self.sizes}, ensemble={self.ensemble}"
