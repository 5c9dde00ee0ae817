"""Shared inputs, float64 reference and error bound of the
``ops.iqn_embedding`` tests, and a seeded ``IQN.update()``. Cached results
are shared: do not modify them.

The reference is the op's definition in float64 from the same fp32
``a = float(i) * taus`` (that product is the one rounding that belongs to
the definition). The bound counts roundings:

* a feature ``c = cos(pi a)``: ``eps_c = |pi a| 2^-23 + 2^-22``, the two
  argument roundings of an fp32 ``cos(pi * a)`` plus 4 ulp for the
  evaluation (a kernel with exact reduction sits far inside);
* ``z``: ``sum_i eps_c |w|`` and ``K + 2`` roundings (K multiply-adds,
  the bias, one spare) of the magnitude sum ``sum_i |c w| + |bias|``;
* ``h = psi max(z, 0)``: ``|psi| z_err`` (ReLU is 1-Lipschitz) and the
  product's rounding ``2^-24 |h|``, ``2^-8 |h|`` more for a bf16 store;
* a gradient summed over ``T`` terms (``N`` for ``dpsi``, ``B N`` for
  ``dweight`` and ``dbias``): the terms' own allowances (``|g| z_err``,
  ``|e| eps_c``) and ``T + 3`` roundings (``T`` additions, up to three
  products per term) of the magnitude sum; ``dpsi`` in bf16 adds
  ``2^-8 |dpsi|``;
* the mask ``[z > 0]`` is discontinuous: an element with ``|z| <= z_err``
  is ambiguous and adds its whole term (``|g psi c|``, for ``dbias``
  ``|g psi|``) to the sums it enters. The tests assert that at most 1e-3
  of the elements are.
"""
import functools
import math
import random
from types import SimpleNamespace

import numpy as np
import torch as t
import torch.nn as nn

# (B, N, D, K): all edge; 15 rows of three samples in one row tile, one
# full and one partial column tile; 66 rows cross a tile inside a sample,
# three column tiles; K off the MFMA step
SHAPES = [(1, 1, 1, 1), (3, 5, 70, 64), (2, 33, 130, 64), (5, 8, 64, 6)]
# forward: 67980 rows are 532 trips of 128 rows against the cap of 512
# row groups (one column chunk), so groups 0-19 make a second trip;
# backward: 1 chunk asks for 512 slices, so 5 samples per slice (wave 0
# takes a second one) in 412 slices; a sample's 33 rows are two row
# tiles; D odd takes the scalar loads and stores
SLICED_SHAPE = (2060, 33, 33, 64)
OUTPUTS = ("h", "dpsi", "dweight", "dbias")
U24 = 2.0 ** -24


@functools.lru_cache(maxsize=None)
def make_case(shape, seed=0):
    B, N, D, K = shape
    gen = t.Generator().manual_seed(seed * 7919 + B * 1009 + N * 31 + D + K)

    def uniform(*size):
        return (t.rand(*size, generator=gen) * 2 - 1) / 8

    return SimpleNamespace(
        shape=shape, taus=t.rand(B, N, generator=gen),
        weight=uniform(D, K), bias=uniform(D),
        psi=t.randn(B, D, generator=gen), dh=t.randn(B, N, D, generator=gen),
    )


@functools.lru_cache(maxsize=None)
def reference64(shape, dtype, seed=0):
    """``(ref, bound, ambiguous share)`` with psi and dh rounded to
    ``dtype`` first."""
    case = make_case(shape, seed)
    B, N, D, K = shape
    psi = case.psi.to(dtype).double().repeat_interleave(N, dim=0)  # [R, D]
    g = case.dh.to(dtype).double().view(B * N, D)
    w, bias = case.weight.double(), case.bias.double()
    a = (case.taus.view(-1, 1) * t.arange(K, dtype=t.float32)).double()
    c = t.cos(math.pi * a)
    eps_c = (math.pi * a).abs() * 2.0 ** -23 + 2.0 ** -22
    z = c @ w.t() + bias
    z_err = eps_c @ w.abs().t() \
        + (K + 2) * U24 * (c.abs() @ w.abs().t() + bias.abs())
    relu = z.clamp_min(0)
    e = g * psi * (z > 0)
    amb = (z.abs() <= z_err) * (g * psi).abs()
    store = 2.0 ** -8 if dtype == t.bfloat16 else 0.0

    def per_sample(x):
        return x.view(B, N, D).sum(dim=1)

    ref = SimpleNamespace(
        h=(psi * relu).view(B, N, D), dpsi=per_sample(g * relu),
        dweight=e.t() @ c, dbias=e.sum(dim=0),
    )
    bound = SimpleNamespace(
        h=(psi.abs() * z_err).view(B, N, D) + (U24 + store) * ref.h.abs(),
        dpsi=per_sample(g.abs() * z_err)
        + (N + 3) * U24 * per_sample((g * relu).abs())
        + store * ref.dpsi.abs(),
        dweight=e.abs().t() @ eps_c + amb.t() @ c.abs()
        + (B * N + 3) * U24 * (e.abs().t() @ c.abs()),
        dbias=amb.sum(dim=0) + (B * N + 3) * U24 * e.abs().sum(dim=0),
    )
    return ref, bound, float((z.abs() <= z_err).double().mean())


def run(fn, case, dtype, device="cpu", psi=None, taus=None):
    """Forward and backward of ``fn(psi, taus, weight, bias)``: a
    namespace of ``OUTPUTS``, detached, on ``device``."""
    psi = (case.psi if psi is None else psi).to(device=device, dtype=dtype)
    psi = psi.clone().requires_grad_(True)
    taus = (case.taus if taus is None else taus).to(device)
    weight = case.weight.to(device).clone().requires_grad_(True)
    bias = case.bias.to(device).clone().requires_grad_(True)
    h = fn(psi, taus, weight, bias)
    h.backward(case.dh.to(device=device, dtype=dtype))
    return SimpleNamespace(h=h.detach(), dpsi=psi.grad, dweight=weight.grad,
                           dbias=bias.grad)


def worst_ratio(got, ref, bound, scale=1.0):
    """Largest ``|got - ref| / (scale * bound)`` over the outputs, with
    the output's name; where the bound is zero the match must be exact."""
    worst, where = 0.0, None
    for name in OUTPUTS:
        g = getattr(got, name).detach().cpu().double()
        r, b = getattr(ref, name), scale * getattr(bound, name)
        assert g.shape == r.shape and bool(t.isfinite(g).all()), name
        err, zero = (g - r).abs(), b == 0
        assert bool((err[zero] == 0).all()), name
        ratio = float((err[~zero] / b[~zero]).max()) if (~zero).any() else 0.0
        if ratio > worst:
            worst, where = ratio, name
    return worst, where


class PixelIQNNet(nn.Module):
    """Tiny conv torso and an IQN head on [B, 4, 16, 16] u8 stacks."""

    def __init__(self, action_num=3, noisy=False):
        super().__init__()
        from machin_amd.model.nets import ImplicitQuantileHead

        self.conv = nn.Conv2d(4, 4, 4, stride=4)
        self.head = ImplicitQuantileHead(64, action_num, hidden=16,
                                         noisy=noisy)

    def forward(self, state, taus):
        a = t.relu(self.conv(state.float() / 255.0)).flatten(1)
        return self.head(a, taus)


def seeded_iqn_update(device="cpu", **options):
    """One seeded ``update()`` of ``IQN`` on a stored pixel episode:
    ``(algo, parameters before, loss)``. SGD, so a parameter moves in
    proportion to its gradient. The fractions are drawn on the CPU for
    either device, so both see the same."""
    from machin_amd.frame.algorithms import IQN

    t.manual_seed(0)
    algo = IQN(
        PixelIQNNet().to(device), PixelIQNNet().to(device), t.optim.SGD,
        quantiles=8, target_quantiles=6, act_quantiles=4, batch_size=8,
        reward_future_steps=3, learning_rate=0.1, **options,
    )
    algo._sample_taus = lambda batch, n, dev: t.rand(batch, n).to(dev)
    gen = t.Generator().manual_seed(1)
    planes = t.randint(0, 256, (16, 16, 16), dtype=t.uint8, generator=gen)
    algo.store_episode([{
        "state": {"state": planes[None, i:i + 4].clone()},
        "action": {"action": t.randint(0, 3, (1, 1), generator=gen)},
        "next_state": {"state": planes[None, i + 1:i + 5].clone()},
        "reward": float(t.randint(-3, 4, (1,), generator=gen)),
        "terminal": i == 11,
    } for i in range(12)])
    before = [p.detach().clone() for p in algo.qnet.parameters()]
    random.seed(7), np.random.seed(7), t.manual_seed(7)
    return algo, before, algo.update()
