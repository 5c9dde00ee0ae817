"""Shared inputs and references for the ``ops.c51_loss`` tests.

Everything returned from the cached functions here is shared between
tests: do not modify it in place.
"""
import functools
import random
from types import SimpleNamespace

import numpy as np
import torch as t
import torch.nn as nn

import util_ops_reference as R
from machin_amd.auto.model_zoo import DistQNet

V_MIN, V_MAX = -10.0, 10.0
DISCOUNTS = (0.99, 0.99 ** 2, 0.99 ** 3)
MIN_GAP = 1e-2

# (B, A, N): all minima; batch no multiple of the waves per block and
# fewer atoms than lanes; atoms just past one wave; atom limit; action
# limit; more rows than one pass of the grid (2048 blocks x 4 waves)
SMALL_SHAPES = [(1, 1, 2), (5, 3, 51), (67, 18, 65), (33, 6, 256),
                (3, 64, 51)]
LARGE_SHAPE = (8200, 3, 51)
ALL_SHAPES = SMALL_SHAPES + [LARGE_SHAPE]
BACKWARD_SHAPES = [(5, 3, 51), (67, 18, 65), (33, 6, 256)]

# the project's projection tolerance (tests/test_ops_gpu.py)
RTOL, ATOL = 1e-4, 1e-3


def shape_id(shape):
    return "x".join(str(s) for s in shape)


def seed_all(seed=0):
    random.seed(seed)
    np.random.seed(seed)
    t.manual_seed(seed)


def _prob(x, from_logits):
    return t.softmax(x, dim=-1) if from_logits else x


def q_values64(next_online, from_logits, v_min=V_MIN, v_max=V_MAX):
    """Expected value of every action in float64, [B, A]."""
    n = next_online.shape[-1]
    z = t.linspace(v_min, v_max, n, dtype=t.float64)
    return (_prob(next_online.double(), from_logits) * z).sum(dim=-1)


@functools.lru_cache(maxsize=None)
def make_case(shape, dtype=t.float32, from_logits=True):
    """Inputs of one case on the CPU, in ``dtype`` (the three
    distributions) and the op's own dtypes (the rest). Asserts that the
    double-DQN action of every sample is decided by a gap of at least
    ``MIN_GAP``, so no row may be left out of any comparison."""
    B, A, N = shape
    gen = t.Generator().manual_seed(B * 100003 + A * 1009 + N)

    def randn(*size):
        return t.randn(*size, generator=gen)

    dist, next_online, next_target = (randn(B, A, N) for _ in range(3))
    rows = t.arange(B)
    star = t.randint(0, A, (B,), generator=gen)
    z = t.linspace(V_MIN, V_MAX, N)
    next_online[rows, star] += 2.0 * z / V_MAX
    case = SimpleNamespace(
        shape=shape, dtype=dtype, from_logits=from_logits,
        action=t.randint(0, A, (B,), generator=gen),
        reward=4.0 * randn(B),
        terminal=(t.rand(B, generator=gen) > 0.8).float(),
        discount=t.tensor(DISCOUNTS, dtype=t.float32)[
            t.randint(0, 3, (B,), generator=gen)
        ],
        g=randn(B),
    )
    for name, logits in (("dist", dist), ("next_online", next_online),
                         ("next_target", next_target)):
        # bf16 logits are rounded first; probabilities are the softmax
        # of the same logits, then stored in dtype
        logits = logits.to(dtype)
        value = logits if from_logits else \
            t.softmax(logits.float(), dim=-1).to(dtype)
        setattr(case, name, value)
    q = q_values64(case.next_online, from_logits)
    if A > 1:
        top2 = q.topk(2, dim=1).values
        gap = float((top2[:, 0] - top2[:, 1]).min())
        assert gap >= MIN_GAP, f"action gap {gap} at {shape}"
    case.best = q.argmax(dim=1)
    return case


def op_args(case, device="cpu", upcast=False, discount=None):
    """Positional arguments of ``ops.c51_loss`` for a case; ``upcast``
    feeds the distributions as fp32 (same values)."""
    def dist(x):
        return (x.float() if upcast else x).to(device)

    return (
        dist(case.dist), case.action.to(device), dist(case.next_online),
        dist(case.next_target), case.reward.to(device),
        case.terminal.to(device),
        case.discount.to(device) if discount is None else discount,
        getattr(case, "v_min", V_MIN), getattr(case, "v_max", V_MAX),
    )


def reference64(case):
    """(loss, proj, best) from the definitions in float64, written
    independently of the fallback: one pass per atom, accumulating with
    index_put_. The support is ``(V_MIN, V_MAX)`` unless the case
    carries its own ``v_min`` and ``v_max``, which are rounded to fp32
    first as the op does."""
    B, A, N = case.shape
    rows = t.arange(B)
    v_min = R.f32(getattr(case, "v_min", V_MIN))
    v_max = R.f32(getattr(case, "v_max", V_MAX))
    z = t.linspace(v_min, v_max, N, dtype=t.float64)
    delta = (v_max - v_min) / (N - 1)
    best = q_values64(case.next_online, case.from_logits, v_min,
                      v_max).argmax(dim=1)
    nd = _prob(case.next_target.double(), case.from_logits)[rows, best]
    gamma = case.discount.double() * (1.0 - case.terminal.double())
    proj = t.zeros(B, N, dtype=t.float64)
    for i in range(N):
        tz = (case.reward.double() + gamma * z[i]).clamp(v_min, v_max)
        pos = (tz - v_min) / delta
        lo, hi = pos.floor(), pos.ceil()
        same = lo == hi
        w_lo = t.where(same, t.ones_like(pos), hi - pos)
        w_hi = t.where(same, t.zeros_like(pos), pos - lo)
        lo_i = lo.long().clamp(0, N - 1)
        hi_i = hi.long().clamp(0, N - 1)
        proj.index_put_((rows, lo_i), nd[:, i] * w_lo, accumulate=True)
        proj.index_put_((rows, hi_i), nd[:, i] * w_hi, accumulate=True)
    pred = case.dist.double()[rows, case.action.clamp(0, A - 1)]
    if case.from_logits:
        log_pred = pred - t.logsumexp(pred, dim=-1, keepdim=True)
    else:
        log_pred = t.log(pred.clamp_min(1e-8))
    return -(proj * log_pred).sum(dim=1), proj, best


@functools.lru_cache(maxsize=None)
def fallback_result(shape, dtype, from_logits):
    """Forward and backward of the CPU fallback on the fp32 upcast of a
    case: ``(loss, proj, best, grad_dist)`` with ``grad_dist`` the fp32
    gradient for the incoming ``case.g``."""
    from machin_amd import ops

    case = make_case(shape, dtype, from_logits)
    args = list(op_args(case, upcast=True))
    args[0] = args[0].clone().requires_grad_(True)
    loss, proj, best = ops._c51_loss_torch(
        *args, from_logits=from_logits
    )
    (grad,) = t.autograd.grad(loss, args[0], case.g)
    return loss.detach(), proj, best, grad


# -- edge cases, the hat-form reference and its rounding bound -------------
U24 = R.U24
# device expf and logf: no ulp figure is documented in the ROCm
# installation the project is built with, so 2 ulp each is assumed
# (1 ulp of v is at most 2 * 2^-24 |v|)
EXP_ULP = LOG_ULP = 2
EPS32 = R.f32(1e-8)  # the kernels' 1e-8f

EDGE_SUPPORTS = R.PROJ_RANGES + [(-3.7, 11.3)]
# all minima; fewer atoms than lanes with a batch no multiple of the
# waves per block; atoms just past one wave; the atom limit; atoms that
# end inside the second wave; the action limit
EDGE_SHAPES = [(1, 1, 2), (5, 3, 51), (67, 18, 65), (33, 6, 256),
               (9, 4, 124), (3, 64, 51)]
OVERSHOOT_BATCH, OVERSHOOT_ACTIONS = 5, 2


def _overshoot_cases():
    """For each range of ``R.PROJ_RANGES`` the smallest and the largest
    atom count at which the fp32 position of ``v_max`` lands above the
    last bin."""
    found = R.overshooting_supports()
    cases = []
    for lo, hi in R.PROJ_RANGES:
        atoms = sorted(a for l, h, a in found if (l, h) == (lo, hi))
        for a in sorted({atoms[0], atoms[-1]} if atoms else ()):
            cases.append(((OVERSHOOT_BATCH, OVERSHOOT_ACTIONS, a), lo, hi))
    return cases


# (shape, v_min, v_max); the large shape (more rows than one forward
# pass of 2048 x 4 row-waves, more elements than one backward pass of
# 2048 x 256 threads) on (-10, 10) only
EDGE_CASES = (
    [(s, lo, hi) for s in EDGE_SHAPES for lo, hi in EDGE_SUPPORTS]
    + _overshoot_cases()
    + [(LARGE_SHAPE, V_MIN, V_MAX)]
)
# the wrong-reference check runs where the batch holds every named row
# and enough random ones
WRONG_CASES = [c for c in EDGE_CASES if c[0][0] >= 33]
WRONG_VARIANTS = ("swap_weights", "drop_last_atom", "ignore_terminal",
                  "constant_discount", "unclamped", "best_as_action")


def edge_id(case_key):
    shape, lo, hi = case_key
    return f"{shape_id(shape)}_{lo:g}_{hi:g}"


@functools.lru_cache(maxsize=None)
def make_edge_case(shape, v_min, v_max, dtype=t.float32, from_logits=True):
    """Like :func:`make_case` on the support ``(v_min, v_max)``, with
    named rows where the batch has them. last: every atom clamps to
    ``v_max`` (reward ``v_max + 2 span``); 0: every atom clamps to
    ``v_min``; 1: terminal, reward exactly on the top atom; 2: terminal
    on the bottom atom; 3: terminal on the interior atom ``v_min32 +
    dz32 * (N // 2)`` formed in fp32; 4: discount 0, not terminal;
    5: discount 1, not terminal; the rest random in ``[v_min - 0.1
    span, v_max + 0.1 span]``, one in five terminal, discounts from
    ``DISCOUNTS``. The double-DQN action of every row is decided by a
    gap of at least ``MIN_GAP`` on a span of 20."""
    B, A, N = shape
    gen = t.Generator().manual_seed(7000 + B * 100003 + A * 1009 + N)

    def randn(*size):
        return t.randn(*size, generator=gen)

    lo32, hi32 = np.float32(v_min), np.float32(v_max)
    lo, hi = float(lo32), float(hi32)
    span = hi - lo
    dist, next_online, next_target = (randn(B, A, N) for _ in range(3))
    rows = t.arange(B)
    star = t.randint(0, A, (B,), generator=gen)
    next_online[rows, star] += t.linspace(-2.0, 2.0, N)
    action = t.randint(0, A, (B,), generator=gen)
    reward = (lo + span * (t.rand(B, generator=gen, dtype=t.float64)
                           * 1.2 - 0.1)).float()
    terminal = (t.rand(B, generator=gen) < 0.2).float()
    discount = t.tensor(DISCOUNTS, dtype=t.float32)[
        t.randint(0, 3, (B,), generator=gen)
    ]
    g = randn(B)
    if B > 1:
        reward[0], terminal[0] = lo - 2 * span, 0.0
    if B > 2:
        reward[1], terminal[1] = hi, 1.0
    if B > 3:
        reward[2], terminal[2] = lo, 1.0
    if B > 4:
        dz32 = (hi32 - lo32) / np.float32(N - 1)
        interior = lo32 + dz32 * np.float32(N // 2)
        assert interior.dtype == np.float32
        reward[3], terminal[3] = float(interior), 1.0
    if B > 5:
        discount[4], terminal[4] = 0.0, 0.0
    if B > 6:
        discount[5], terminal[5] = 1.0, 0.0
    reward[B - 1], terminal[B - 1] = hi + 2 * span, 0.0
    case = SimpleNamespace(
        shape=shape, dtype=dtype, from_logits=from_logits, v_min=v_min,
        v_max=v_max, action=action, reward=reward, terminal=terminal,
        discount=discount, g=g,
    )
    for name, logits in (("dist", dist), ("next_online", next_online),
                         ("next_target", next_target)):
        logits = logits.to(dtype)
        value = logits if from_logits else \
            t.softmax(logits.float(), dim=-1).to(dtype)
        setattr(case, name, value)
    q = q_values64(case.next_online, from_logits, lo, hi)
    if A > 1:
        top2 = q.topk(2, dim=1).values
        gap = float((top2[:, 0] - top2[:, 1]).min()) * 20.0 / span
        assert gap >= MIN_GAP, f"action gap {gap} at {shape}"
    case.best = q.argmax(dim=1)
    return case


@functools.lru_cache(maxsize=None)
def make_tie_case(dtype=t.float32, from_logits=True):
    """The ``(9, 4, 124)`` edge case on ``(-10, 10)`` with, in every
    row, the maximal ``next_online`` row copied bit for bit over one
    other action, below or above it: ``best`` must be the lower of the
    two. The target net's rows of the two actions differ, so in the
    random rows the choice shows in ``proj`` too."""
    src = make_edge_case((9, 4, 124), V_MIN, V_MAX, dtype, from_logits)
    case = SimpleNamespace(**vars(src))
    case.next_online = src.next_online.clone()
    want, above = [], 0
    for b in range(9):
        star = int(src.best[b])
        other = (star + 1 + b % 3) % 4
        case.next_online[b, other] = src.next_online[b, star]
        want.append(min(star, other))
        above += other > star
    assert 0 < above < 9  # both orders occur
    case.best = t.tensor(want)
    return case


def reference_hat(case, wrong=None):
    """``(ref, bound)``: the op in float64 in hat form, and the
    worst-case error of an fp32 evaluation of it in any order.

    ``ref`` holds ``loss [B]``, ``proj [B, N]``, ``best [B]`` and
    ``grad [B, N]``, the gradient with respect to the taken row
    ``dist[b, a_b]`` for the incoming ``case.g``. The form differs from
    the kernel, the fallback and :func:`reference64` (floor, ceil and
    two scatters): with ``hat(x) = max(0, 1 - |x|)``, one source atom at
    a time, ::

        proj[b, j] = sum_i p[b, i] hat(pos[b, i] - j)
        pos[b, i]  = (clamp(r_b + gamma_b z_i, v_min, v_max) - v_min)
                     (N - 1) / span

    in float64 from the fp32-rounded ``v_min``, ``v_max``, reward,
    discount and terminal (``gamma = discount (1 - terminal)``, ``z_i =
    v_min + i span / (N - 1)``). ``tz`` is clamped first; weight of a
    position past bin ``N - 1`` is folded into bin ``N - 1``.
    Gradient: ``g (softmax(dist) sum(proj) - proj)`` for logits,
    ``-g proj / dist`` where ``dist >= 1e-8f`` (else 0) for
    probabilities. The inputs are taken as stored (a bf16 case starts
    from the bf16-rounded values).

    The bound counts roundings, to first order in ``u = 2^-24``, of the
    kernels' operation sequence (machin_amd/ops/hip/c51_loss.hip); the
    fallback's sequence has the same counts. ``hat`` is 1-Lipschitz, so
    a position error ``E`` moves at most ``p E`` of mass in each bin
    within ``1 + E`` of the position, also when it flips floor and
    ceil; the fold keeps that true at the top bin.

    * ``dz32 = fl(fl(v_max - v_min) / (N - 1))``: 2 roundings. The
      fallback divides in float64 from the unrounded ends and rounds
      once; the ends move the span by at most ``u (|v_min| + |v_max|)``.
      Relative error of ``dz``: ``k u`` with ``k = 1 + max(1, (|v_min|
      + |v_max|) / span)``, 2 on every support that contains 0.
    * ``z_i = fl(v_min + fl(dz32 i))``: ``|dz_i| <= 3 u i dz + u |z_i|
      <= 4 u Z``, ``Z = max(|v_min|, |v_max|, span)``.
    * ``g = fl(discount fl(1 - terminal))``: relative ``2 u``.
    * ``tz_i = fl(r + fl(g z_i))``: ``|g| 4 u Z`` (z) ``+ 2 u |g z|``
      (g) ``+ u |g z|`` (product) ``+ u |tz|`` (sum, ``|tz| <= |r| +
      |g| Z``): ``|dtz_i| <= u (|r| + 8 |gamma| Z)``, i.e. ``c1 = 8``
      on the discounted term and 1 on the reward. Where the unclamped
      float64 target lies outside ``[v_min, v_max]`` by more than that,
      both evaluations clamp to the same end: ``dtz_i = 0``. The clamp
      is exact (the ends are fp32) and 1-Lipschitz elsewhere.
    * ``pos = fl(fl(tz - v_min) / dz32)``: ``u span / dz`` (difference)
      ``+ (k + 1) u (N - 1)`` (dz32, division): ``E_i = (dtz_i + u span)
      / dz + c2 u (N - 1)`` capped at 1, ``c2 = k + 1 = 3``. floor and
      ceil are exact.
    * softmax (logits only), ``p_i = expf(fl(x_i - lse))`` with ``lse =
      fl(m + logf(s))``, ``s = sum_k expf(fl(x_k - m))``: each term of
      ``s`` has relative error ``u |x_k - m| + 2 EXP_ULP u``, the sum
      adds ``(N - 1) u``, so ``s`` is off by at most ``(D + 2 EXP_ULP
      + N - 1) u`` relative with ``D = sum_k p_k |x_k - m|``; logf adds
      ``2 LOG_ULP u |lse - m|`` and the last sum ``u |lse|``. With the
      argument rounding ``u |x_i - lse|`` and expf's own error::

          rho_i = (|x_i - lse| + |lse| + 2 LOG_ULP |lse - m| + D + N
                   + c3) u,  c3 = 4 EXP_ULP - 1 = 7

      (the fallback's ``expf(x_i - m) / s`` needs ``|x_i - m| <=
      |x_i - lse| + |lse - m|`` and one division, covered by the logf
      term and c3). Probabilities: ``rho = 0``.
    * weights and accumulation: ``hi_f - pos`` is exact unless ``pos <
      1`` (1 rounding), the product ``p w`` 1, at most ``N - 1`` sums
      per bin, one unit kept for the second order: ``N + c4``,
      ``c4 = 2``. ::

          bound.proj[j] = sum_i p_i E_i [|pos_i - j| < 1 + E_i]
                          + u sum_i (rho_i + N + c4) p_i hat_ij

    * loss, ``-sum_j proj_j logp_j``: ``dlogp_j = u |logp_j| + dlse``
      for logits (``logp = fl(x - lse)``, ``dlse`` the error of the
      taken row's lse from the softmax item) and ``2 LOG_ULP u
      |logp_j|`` for probabilities; each product 1 rounding, at most
      ``N - 1`` sums, one unit for the second order (``c5 = 2``)::

          bound.loss = sum_j (bound.proj_j |logp_j| + proj_j dlogp_j)
                       + (N + c5) u sum_j |proj_j logp_j|

    * gradient, logits, ``fl(g fl(fl(expf(fl(x - lse)) S) - proj))``
      with the stored fp32 ``lse`` and ``S``: ``dS = sum_j bound.proj_j
      + (N - 1) u S``; the product with ``S`` 1 rounding; the
      difference and the product with ``g`` are relative to the
      result (``c = 2``)::

          bound.grad = |g| ((rho_j + u) p_j S + p_j dS + bound.proj_j)
                       + 2 u |grad|

    * gradient, probabilities, ``fl(fl(-g proj) / dist)``::

          bound.grad = |g| bound.proj_j / dist_j + 2 u |grad|

    * a bf16 gradient adds ``2^-8 |grad|``.

    ``wrong`` names one deliberately wrong variant (``WRONG_VARIANTS``)
    for the test that the bound tells them from the truth; the bound
    returned with a variant is meaningless. ``"unclamped"`` leaves
    ``tz`` unclamped and sums only over the bins that exist, without
    the fold: in floor-and-ceil form the two weights always sum to 1,
    so clamping the indices alone would reproduce the clamp exactly;
    what a kernel without the clamp can lose is the mass whose bins lie
    outside. No variant drops ``S = sum(proj)`` from the logits
    gradient: the rows are normalised, ``S`` is 1 and dropping it is
    not observable here.
    """
    assert wrong is None or wrong in WRONG_VARIANTS
    B, A, N = case.shape
    logits = case.from_logits
    u = U24
    lo = R.f32(getattr(case, "v_min", V_MIN))
    hi = R.f32(getattr(case, "v_max", V_MAX))
    span = hi - lo
    dz = span / (N - 1)
    Z = max(abs(lo), abs(hi), span)
    k = 1.0 + max(1.0, (abs(lo) + abs(hi)) / span)
    c2, c3, c4, c5 = k + 1.0, 4 * EXP_ULP - 1, 2, 2
    rows = t.arange(B)
    j = t.arange(N, dtype=t.float64).view(1, N)
    z = lo + span * j / (N - 1)

    def softmax_terms(x):
        """p, log p, rho and the lse error of logits rows [B, N]."""
        m = x.max(dim=1, keepdim=True).values
        lse = t.logsumexp(x, dim=1, keepdim=True)
        logp = x - lse
        p = t.exp(logp)
        D = (p * (x - m).abs()).sum(dim=1, keepdim=True)
        dlse = u * (D + 2 * EXP_ULP + N - 1
                    + 2 * LOG_ULP * (lse - m).abs() + lse.abs())
        rho = u * (logp.abs() + 2 * EXP_ULP) + dlse
        return p, logp, rho, dlse

    # double-DQN action: the first maximal q
    x_on = case.next_online.double()
    p_on = t.softmax(x_on, dim=-1) if logits else x_on
    best = (p_on * z.view(1, 1, N)).sum(dim=-1).argmax(dim=1)

    x_t = case.next_target.double()[rows, best]
    if logits:
        p, _, rho, _ = softmax_terms(x_t)
    else:
        p, rho = x_t, t.zeros_like(x_t)
    if wrong == "drop_last_atom":
        p = p.clone()
        p[:, N - 1] = 0.0

    r = case.reward.double().view(B, 1)
    alive = 1.0 - case.terminal.double().view(B, 1)
    discount = case.discount.double().view(B, 1)
    if wrong == "ignore_terminal":
        alive = t.ones_like(alive)
    if wrong == "constant_discount":
        discount = t.full_like(discount, R.f32(DISCOUNTS[0]))
    gamma = discount * alive
    tz = r + gamma * z
    dtz = (u * (r.abs() + 8.0 * gamma.abs() * Z)).expand(B, N)
    absorbed = (tz > hi + dtz) | (tz < lo - dtz)
    dtz = t.where(absorbed, t.zeros_like(dtz), dtz)
    if wrong != "unclamped":
        tz = tz.clamp(lo, hi)
    pos = (tz - lo) * (N - 1) / span
    if wrong == "swap_weights":
        pos = pos.floor() + pos.ceil() - pos
    E = ((dtz + u * span) / dz + c2 * u * (N - 1)).clamp(max=1.0)

    proj = t.zeros(B, N, dtype=t.float64)
    bproj = t.zeros(B, N, dtype=t.float64)
    for i in range(N):
        pos_i, p_i, E_i = pos[:, i:i + 1], p[:, i:i + 1], E[:, i:i + 1]
        d = (pos_i - j).abs()
        hat = (1.0 - d).clamp_min(0.0)
        if wrong != "unclamped":
            hat[:, N - 1] = t.where(pos_i[:, 0] > N - 1,
                                    t.ones(B, dtype=t.float64),
                                    hat[:, N - 1])
        proj += p_i * hat
        bproj += p_i * E_i * (d < 1.0 + E_i) \
            + u * (rho[:, i:i + 1] + N + c4) * p_i * hat

    a_b = best if wrong == "best_as_action" else case.action.clamp(0, A - 1)
    xd = case.dist.double()[rows, a_b]
    g = case.g.double().view(B, 1)
    if logits:
        pd, logp, rho_d, dlse_d = softmax_terms(xd)
        dlogp = u * logp.abs() + dlse_d
    else:
        logp = t.log(xd.clamp_min(EPS32))
        dlogp = 2 * LOG_ULP * u * logp.abs()
    terms = proj * logp
    loss = -terms.sum(dim=1)
    bloss = (bproj * logp.abs() + proj * dlogp).sum(dim=1) \
        + (N + c5) * u * terms.abs().sum(dim=1)
    if logits:
        S = proj.sum(dim=1, keepdim=True)
        dS = bproj.sum(dim=1, keepdim=True) + (N - 1) * u * S
        grad = g * (pd * S - proj)
        bgrad = g.abs() * ((rho_d + u) * pd * S + pd * dS + bproj) \
            + 2 * u * grad.abs()
    else:
        kept = xd >= EPS32
        safe = t.where(kept, xd, t.ones_like(xd))
        zero = t.zeros_like(xd)
        grad = t.where(kept, -g * proj / safe, zero)
        bgrad = t.where(kept, g.abs() * bproj / safe + 2 * u * grad.abs(),
                        zero)
    if case.dtype == t.bfloat16:
        bgrad = bgrad + 2.0 ** -8 * grad.abs()
    ref = SimpleNamespace(loss=loss, proj=proj, best=best, grad=grad)
    bound = SimpleNamespace(loss=bloss, proj=bproj, grad=bgrad)
    return ref, bound


@functools.lru_cache(maxsize=None)
def edge_reference(case_key, dtype, from_logits):
    """:func:`reference_hat` of an edge case, shared between tests."""
    return reference_hat(make_edge_case(*case_key, dtype, from_logits))


def taken_rows(grad, case):
    """``[B, N]`` rows of the taken actions of a ``[B, A, N]`` gradient
    and whether every other row is exactly zero."""
    B, A, _ = case.shape
    a_b = case.action.clamp(0, A - 1)
    taken = t.zeros(B, A, dtype=t.bool)
    taken[t.arange(B), a_b] = True
    return grad[t.arange(B), a_b], bool((grad[~taken] == 0).all())


def fallback_edge_result(case):
    """Forward and autograd backward of the fp32 CPU fallback on a case:
    ``(loss, proj, best, grad [B, A, N])``."""
    from machin_amd import ops

    args = list(op_args(case, upcast=True))
    args[0] = args[0].clone().requires_grad_(True)
    loss, proj, best = ops._c51_loss_torch(
        *args, from_logits=case.from_logits
    )
    (grad,) = t.autograd.grad(loss, args[0], case.g)
    return loss.detach(), proj, best, grad


def worst_ratio(got, want64, bound):
    """``(max err / bound, all within)`` of an fp32 or bf16 result."""
    err = (got.detach().cpu().double() - want64).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    return ratio, bool((err <= bound).all())


# -- RAINBOW helpers -------------------------------------------------------
class LogitsQNet(DistQNet):
    """The model-zoo distributional MLP without its softmax."""

    def forward(self, state):
        a = t.relu(self.fc1(state))
        return self.fc2(a).view(-1, self.action_num, self.atom_num)


def vector_episode(length=20, seed=1):
    gen = t.Generator().manual_seed(seed)
    return [
        {
            "state": {"state": t.rand(1, 4, generator=gen)},
            "action": {"action": t.randint(0, 2, (1, 1), generator=gen)},
            "next_state": {"state": t.rand(1, 4, generator=gen)},
            "reward": float(t.randn(1, generator=gen)),
            "terminal": i == length - 1,
        }
        for i in range(length)
    ]


def build_rainbow(device="cpu", net=DistQNet, **options):
    """Same seed, same weights, same stored episode for every call."""
    from machin_amd.frame.algorithms import RAINBOW

    seed_all(0)
    algo = RAINBOW(
        net().to(device), net().to(device), t.optim.Adam, V_MIN, V_MAX,
        batch_size=16, reward_future_steps=3, **options,
    )
    algo.store_episode(vector_episode())
    return algo


def seeded_update(algo):
    seed_all(7)
    return algo.update()


class PixelDistQNet(nn.Module):
    """Tiny C51 net on [B, 4, 4, 8] u8 stacks."""

    def __init__(self, action_num=3, atom_num=11):
        super().__init__()
        self.action_num, self.atom_num = action_num, atom_num
        self.fc = nn.Linear(4 * 4 * 8, action_num * atom_num)

    def forward(self, state):
        a = self.fc(state.float().flatten(1) / 255.0)
        return t.softmax(a.view(-1, self.action_num, self.atom_num), dim=-1)


def pixel_episode(length, h=4, w=8, k=4, seed=0):
    """Raw sliding-window episode that ends WITHOUT a terminal (a time
    limit): its last windows are cut short and still bootstrap."""
    gen = t.Generator().manual_seed(seed)
    planes = t.randint(0, 256, (length + k, h, w), dtype=t.uint8,
                       generator=gen)
    return [
        {
            "state": {"state": planes[i : i + k].clone().unsqueeze(0)},
            "action": {"action": t.randint(0, 3, (1, 1), generator=gen)},
            "next_state": {
                "state": planes[i + 1 : i + k + 1].clone().unsqueeze(0)
            },
            "reward": float(t.randint(-3, 4, (1,), generator=gen)),
            "terminal": False,
        }
        for i in range(length)
    ]


class FixedLogitsNet(nn.Module):
    """Returns the same ``[A, N]`` logits for every state: 2 actions, 3
    atoms on the support ``(-10, 0, 10)``. Softmaxed, action 0 is worth
    8.6 and action 1 is worth 5.0; read as if the logits were
    probabilities, action 0 would be worth 30 and action 1 200. So the
    greedy action is 0 only if the softmax is applied."""

    def __init__(self):
        super().__init__()
        self.table = nn.Parameter(
            t.tensor([[0.0, 0.0, 3.0], [-20.0, 0.0, 0.0]])
        )

    def forward(self, state):
        return self.table.unsqueeze(0).expand(state.shape[0], 2, 3)


def record_update(monkeypatch, algo):
    """Wrap ``ops.c51_loss`` and the buffer's ``sample_batch`` for the
    coming ``algo.update()`` calls; returns the list that receives one
    ``SimpleNamespace(args, kwargs, out, is_weight, index)`` per
    update."""
    from machin_amd import ops

    calls, samples = [], []
    real_loss = ops.c51_loss
    real_sample = algo.replay_buffer.sample_batch

    def sample_batch(*args, **kwargs):
        out = real_sample(*args, **kwargs)
        samples.append(out)
        return out

    def c51_loss(*args, **kwargs):
        out = real_loss(*args, **kwargs)
        sample = samples[-1]
        calls.append(SimpleNamespace(
            args=args, kwargs=kwargs, out=out, index=sample[2],
            is_weight=t.as_tensor(sample[3]).detach().cpu().double(),
        ))
        return out

    monkeypatch.setattr(algo.replay_buffer, "sample_batch", sample_batch)
    monkeypatch.setattr(ops, "c51_loss", c51_loss)
    return calls


def expected_logits_loss(call):
    """The loss ``update()`` must return for a recorded call when the
    model's outputs are logits: the IS-weighted mean of
    ``-sum(proj * log_softmax)`` from :func:`reference64` (float64, on
    the CPU) over the tensors that reached ``ops.c51_loss``."""
    dist, action, next_online, next_target, reward, terminal, discount = (
        x.detach().cpu() if t.is_tensor(x) else x for x in call.args[:7]
    )
    B = dist.shape[0]
    if not t.is_tensor(discount):
        discount = t.full((B,), float(discount), dtype=t.float64)
    assert tuple(call.args[7:9]) == (V_MIN, V_MAX)
    case = SimpleNamespace(
        shape=tuple(dist.shape), from_logits=True, dist=dist,
        action=action.view(B), next_online=next_online,
        next_target=next_target, reward=reward.float().view(B),
        terminal=terminal.float().view(B), discount=discount.view(B),
    )
    per_sample, _, _ = reference64(case)
    return float((per_sample * call.is_weight.view(B)).mean())
