"""machin_amd.ops — gfx950 HIP kernels with CPU fallbacks.

Every hot data-path op identified in SURVEY.md §2.6-B has two
implementations:

* a hand-written CDNA4 HIP kernel (``machin_amd/ops/hip/*.hip``),
  compiled in-tree into the ``machin_amd.ops._machin_hip`` extension
  (``setup.py build_ext --inplace`` with ``PYTORCH_ROCM_ARCH=gfx950``);
* a pure-PyTorch fallback used on CPU.

Dispatch policy: CUDA tensors REQUIRE the extension — if it is missing
on a GPU machine we raise instead of silently falling back to eager
torch, so a benchmark can never accidentally measure the fallback.
"""
import os
from typing import List, Optional, Sequence

import torch as t

_ext = None
_ext_error: Optional[str] = None


def _use_fused_polyak() -> bool:
    return os.environ.get("MACHIN_AMD_FUSED_POLYAK", "0") == "1"


class FusedPolyak:
    """Precomputed single-launch polyak update over a parameter list.

    The round-1 kernel lost to torch ``_foreach`` (0.106 vs 0.017 ms,
    profiles/kernel_bench_r01.json) because every call rebuilt the
    pointer table on the host and shipped it H2D. This plan builds the
    device table ONCE; each call is one kernel launch with zero host
    setup. Construction raises ValueError if any tensor pair is not
    eligible (contiguous fp32 CUDA) — callers fall back to _foreach.
    """

    def __init__(self, targets: List[t.Tensor], sources: List[t.Tensor]):
        ext = _require_ext()
        n = len(targets)
        if n == 0:
            raise ValueError("empty tensor list")
        for tt, ss in zip(targets, sources):
            if not (
                tt.is_cuda and ss.is_cuda
                and tt.is_contiguous() and ss.is_contiguous()
                and tt.dtype == t.float32 and ss.dtype == t.float32
                and tt.numel() == ss.numel()
            ):
                raise ValueError("ineligible tensor pair for fused polyak")
        table = t.empty(3 * n + 1, dtype=t.int64)
        total = 0
        for i, (tt, ss) in enumerate(zip(targets, sources)):
            table[2 * i] = tt.data_ptr()
            table[2 * i + 1] = ss.data_ptr()
            table[2 * n + i] = total
            total += tt.numel()
        table[3 * n] = total
        self.table = table.to(targets[0].device)
        self.n = n
        self.total = total
        self._sig = tuple(int(x.data_ptr()) for x in targets) + tuple(
            int(x.data_ptr()) for x in sources
        )
        self._ext = ext

    def matches(self, targets, sources) -> bool:
        """Cheap revalidation: storage pointers unchanged."""
        if len(targets) != self.n:
            return False
        sig = tuple(int(x.data_ptr()) for x in targets) + tuple(
            int(x.data_ptr()) for x in sources
        )
        return sig == self._sig

    def __call__(self, tau: float):
        self._ext.multi_tensor_polyak_cached(
            self.table, self.n, self.total, float(tau)
        )


class FusedRMSprop:
    """Cached-plan fused gradient-clip + RMSprop step (two kernel
    launches, zero host synchronization — the eager
    ``clip_grad_norm_`` + foreach-RMSprop chain is ~10 launches with
    the clip threshold bouncing through device scalars).

    Build from a ``torch.optim.RMSprop`` whose state is materialized
    (run one eager step first); semantics match momentum=0,
    centered=False, weight_decay=0 plus ``clip_grad_norm_(max_norm)``
    (pass ``max_norm<=0`` to skip clipping). Parameters, grads and
    ``square_avg`` state are updated in place through a precomputed
    device pointer table.
    """

    def __init__(self, optimizer: "t.optim.RMSprop",
                 max_norm: float = 0.0):
        ext = _require_ext()
        group = optimizer.param_groups[0]
        if (
            group.get("momentum", 0) != 0
            or group.get("centered", False)
            or group.get("weight_decay", 0) != 0
            or len(optimizer.param_groups) != 1
        ):
            raise ValueError(
                "FusedRMSprop supports a single param group with "
                "momentum=0, centered=False, weight_decay=0."
            )
        self.lr = float(group["lr"])
        self.alpha = float(group["alpha"])
        self.eps = float(group["eps"])
        self.max_norm = float(max_norm)
        params = [p for p in group["params"] if p.requires_grad]
        trips = []
        for p in params:
            st = optimizer.state.get(p)
            if st is None or "square_avg" not in st:
                raise ValueError(
                    "optimizer state not materialized; run one eager "
                    "step first"
                )
            g, sq = p.grad, st["square_avg"]
            for x in (p, g, sq):
                if not (
                    x is not None and x.is_cuda and x.is_contiguous()
                    and x.dtype == t.float32
                ):
                    raise ValueError(
                        "FusedRMSprop needs contiguous fp32 CUDA "
                        "params/grads/state"
                    )
            trips.append((p.data, g, sq))
        n = len(trips)
        table = t.empty(4 * n + 1, dtype=t.int64)
        total = 0
        for i, (pd, g, sq) in enumerate(trips):
            table[3 * i] = pd.data_ptr()
            table[3 * i + 1] = g.data_ptr()
            table[3 * i + 2] = sq.data_ptr()
            table[3 * n + i] = total
            total += pd.numel()
        table[4 * n] = total
        dev = trips[0][0].device
        self.table = table.to(dev)
        self.norm_buf = t.zeros(1, dtype=t.float32, device=dev)
        self.n = n
        self.total = total
        self._sig = tuple(
            int(x.data_ptr()) for tr in trips for x in tr
        )
        self._ext = ext

    def matches(self, optimizer) -> bool:
        group = optimizer.param_groups[0]
        sig = []
        for p in group["params"]:
            if not p.requires_grad:
                continue
            st = optimizer.state.get(p)
            if st is None or p.grad is None:
                return False
            sig += [int(p.data.data_ptr()), int(p.grad.data_ptr()),
                    int(st["square_avg"].data_ptr())]
        return tuple(sig) == self._sig

    def step(self):
        self._ext.fused_rmsprop_cached(
            self.table, self.n, self.total, self.norm_buf,
            self.max_norm, self.lr, self.alpha, self.eps,
        )


def _load_ext():
    global _ext, _ext_error
    if _ext is not None or _ext_error is not None:
        return _ext
    try:
        from . import _machin_hip  # type: ignore

        _ext = _machin_hip
    except ImportError as e:
        _ext_error = str(e)
    return _ext


def available() -> bool:
    """True if the gfx950 HIP extension is importable."""
    return _load_ext() is not None


def _require_ext():
    ext = _load_ext()
    if ext is None:
        raise RuntimeError(
            "machin_amd HIP extension is not built but a CUDA tensor was "
            "passed. Build it in-tree with: python setup.py build_ext "
            f"--inplace  (import error: {_ext_error})"
        )
    return ext


# ======================================================================
# fused multi-tensor polyak update (soft_update hot path)
# ======================================================================
def polyak_update_(
    targets: List[t.Tensor], sources: List[t.Tensor], tau: float
) -> None:
    """target = target*(1-tau) + source*tau, fused over all tensors.

    Replaces the per-parameter python loop of the reference
    (machin/frame/algorithms/utils.py:8-27) with one HIP kernel pass
    over every parameter chunk (HBM-bound: one read+write of target,
    one read of source).
    """
    if not targets:
        return
    if not _use_fused_polyak():
        # round-1 measurement (profiles/kernel_bench_r01.json): the v1
        # HIP kernel was 6× slower than torch _foreach on small param
        # sets (one launch per chunk list rebuild), so _foreach is the
        # default until the fused kernel measures faster; flip with
        # MACHIN_AMD_FUSED_POLYAK=1 after building the v2 kernel.
        t._foreach_mul_(targets, 1.0 - tau)
        t._foreach_add_(targets, sources, alpha=tau)
        return
    fused_t, fused_s, plain_t, plain_s = [], [], [], []
    for tt, ss in zip(targets, sources):
        # the HIP kernel walks flat storage: standard-contiguous
        # fp32 pairs only (channels_last params etc. take _foreach)
        if (
            tt.is_cuda
            and tt.is_contiguous()
            and ss.is_contiguous()
            and tt.dtype == t.float32
            and ss.dtype == t.float32
        ):
            fused_t.append(tt)
            fused_s.append(ss)
        else:
            plain_t.append(tt)
            plain_s.append(ss)
    if fused_t:
        ext = _require_ext()
        ext.multi_tensor_polyak(fused_t, fused_s, float(tau))
    if plain_t:
        t._foreach_mul_(plain_t, 1.0 - tau)
        t._foreach_add_(plain_t, plain_s, alpha=tau)


# ======================================================================
# reverse-time scans: discounted returns, GAE, n-step, V-trace
# ======================================================================
def discounted_returns(
    rewards: t.Tensor,
    terminals: t.Tensor,
    gamma: float,
    bootstrap: Optional[t.Tensor] = None,
) -> t.Tensor:
    """R_t = r_t + gamma * (1-d_t) * R_{t+1}; shape [T] or [T, B].

    Reference semantics: machin/frame/algorithms/a2c.py:275-313 (the
    lambda==1 GAE branch).
    """
    rewards = rewards.float()
    squeeze = rewards.dim() == 1
    if squeeze:
        rewards = rewards.unsqueeze(1)
        terminals = terminals.view(-1, 1)
        if bootstrap is not None:
            bootstrap = bootstrap.view(1)
    T, B = rewards.shape
    terminals = terminals.view(T, B).to(rewards.dtype)
    if bootstrap is None:
        bootstrap = t.zeros(B, dtype=rewards.dtype, device=rewards.device)
    if rewards.is_cuda:
        ext = _require_ext()
        out = ext.discounted_returns(
            rewards.contiguous(), (1.0 - terminals).contiguous(),
            bootstrap.contiguous().float(), float(gamma),
        )
    else:
        out = t.empty_like(rewards)
        running = bootstrap.clone().to(rewards.dtype)
        for i in range(T - 1, -1, -1):
            running = rewards[i] + gamma * (1.0 - terminals[i]) * running
            out[i] = running
    return out.squeeze(1) if squeeze else out


def gae(
    rewards: t.Tensor,
    values: t.Tensor,
    next_values: t.Tensor,
    terminals: t.Tensor,
    gamma: float,
    lam: float,
) -> t.Tensor:
    """Generalized advantage estimation; shapes [T] or [T, B].

    A_t = delta_t + gamma*lam*(1-d_t)*A_{t+1},
    delta_t = r_t + gamma*(1-d_t)*V_{t+1} - V_t.
    Reference semantics: machin/frame/algorithms/a2c.py:269-326.
    """
    squeeze = rewards.dim() == 1
    rewards = rewards.float()
    if squeeze:
        rewards = rewards.unsqueeze(1)
        values = values.view(-1, 1)
        next_values = next_values.view(-1, 1)
        terminals = terminals.view(-1, 1)
    T, B = rewards.shape
    values = values.view(T, B).float()
    next_values = next_values.view(T, B).float()
    terminals = terminals.view(T, B).to(rewards.dtype)
    if rewards.is_cuda:
        ext = _require_ext()
        out = ext.gae(
            rewards.contiguous(), values.contiguous(),
            next_values.contiguous(), (1.0 - terminals).contiguous(),
            float(gamma), float(lam),
        )
    else:
        nd = 1.0 - terminals
        delta = rewards + gamma * nd * next_values - values
        out = t.empty_like(delta)
        running = t.zeros(B, dtype=rewards.dtype, device=rewards.device)
        for i in range(T - 1, -1, -1):
            running = delta[i] + gamma * lam * nd[i] * running
            out[i] = running
    return out.squeeze(1) if squeeze else out


def nstep_returns(
    rewards: t.Tensor, terminals: t.Tensor, gamma: float, n: int
) -> t.Tensor:
    """n-step truncated return per timestep; shape [T] or [T, B].

    G_t = sum_{k=0}^{n-1} gamma^k r_{t+k} (stopping at terminal).
    Reference semantics: machin/frame/algorithms/rainbow.py:179-189.
    """
    squeeze = rewards.dim() == 1
    rewards = rewards.float()
    if squeeze:
        rewards = rewards.unsqueeze(1)
        terminals = terminals.view(-1, 1)
    T, B = rewards.shape
    alive = 1.0 - terminals.view(T, B).to(rewards.dtype)
    if rewards.is_cuda:
        ext = _require_ext()
        out = ext.nstep_returns(
            rewards.contiguous(), alive.contiguous(), float(gamma), int(n)
        )
        return out.squeeze(1) if squeeze else out
    # vectorized recurrence (no python per-timestep loop, VERDICT
    # round-1 weak #5): H^{(m)}_t = r_t + gamma*a_t*H^{(m-1)}_{t+1},
    # H^{(0)} = 0, truncating at the sequence end.  n full-tensor
    # passes instead of O(T*n) per-element python work.
    pad = t.zeros(1, B, dtype=rewards.dtype, device=rewards.device)
    out = t.zeros_like(rewards)
    for _ in range(max(1, int(n))):
        out = rewards + gamma * alive * t.cat([out[1:], pad], dim=0)
    return out.squeeze(1) if squeeze else out


def vtrace(
    behavior_log_probs: t.Tensor,
    target_log_probs: t.Tensor,
    rewards: t.Tensor,
    values: t.Tensor,
    bootstrap_value: t.Tensor,
    terminals: t.Tensor,
    gamma: float,
    rho_clip: float = 1.0,
    c_clip: float = 1.0,
    pg_rho_clip: float = 1.0,
    time_major: bool = True,
):
    """IMPALA V-trace targets; shapes [T, B] (or [B, T] with
    ``time_major=False`` — the batch-major kernel lets segment-major
    HBM pools feed the update with zero-copy gathers).

    Returns (vs, pg_advantages) in the input layout, both detached.
    Reference semantics: machin/frame/algorithms/impala.py:317-371.
    """
    if not time_major:
        if rewards.is_cuda:
            ext = _require_ext()
            B, T = rewards.shape
            vs, pg_adv = ext.vtrace_bt(
                behavior_log_probs.detach().float().contiguous(),
                target_log_probs.detach().float().contiguous(),
                rewards.detach().float().contiguous(),
                values.detach().float().contiguous(),
                bootstrap_value.detach().float().contiguous(),
                (1.0 - terminals.detach().float()).contiguous(),
                float(gamma), float(rho_clip), float(c_clip),
                float(pg_rho_clip),
            )
            return vs, pg_adv
        vs, pg_adv = vtrace(
            behavior_log_probs.t(), target_log_probs.t(), rewards.t(),
            values.t(), bootstrap_value, terminals.t(), gamma,
            rho_clip, c_clip, pg_rho_clip,
        )
        return vs.t().contiguous(), pg_adv.t().contiguous()
    T, B = rewards.shape
    blp = behavior_log_probs.detach().float().view(T, B)
    tlp = target_log_probs.detach().float().view(T, B)
    rewards = rewards.detach().float().view(T, B)
    values = values.detach().float().view(T, B)
    bootstrap_value = bootstrap_value.detach().float().view(B)
    nd = 1.0 - terminals.detach().float().view(T, B)
    if rewards.is_cuda:
        ext = _require_ext()
        vs, pg_adv = ext.vtrace(
            blp.contiguous(), tlp.contiguous(), rewards.contiguous(),
            values.contiguous(), bootstrap_value.contiguous(), nd.contiguous(),
            float(gamma), float(rho_clip), float(c_clip), float(pg_rho_clip),
        )
        return vs, pg_adv
    rho = t.exp(tlp - blp)
    clipped_rho = rho.clamp(max=rho_clip)
    cs = rho.clamp(max=c_clip)
    next_values = t.cat([values[1:], bootstrap_value.unsqueeze(0)], dim=0)
    deltas = clipped_rho * (rewards + gamma * nd * next_values - values)
    acc = t.zeros(B, dtype=rewards.dtype)
    vs_minus_v = t.empty_like(values)
    for i in range(T - 1, -1, -1):
        acc = deltas[i] + gamma * nd[i] * cs[i] * acc
        vs_minus_v[i] = acc
    vs = vs_minus_v + values
    vs_next = t.cat([vs[1:], bootstrap_value.unsqueeze(0)], dim=0)
    pg_adv = rho.clamp(max=pg_rho_clip) * (rewards + gamma * nd * vs_next - values)
    return vs, pg_adv


# ======================================================================
# distributional RL: categorical (C51) projection
# ======================================================================
def categorical_projection(
    next_dist: t.Tensor,
    rewards: t.Tensor,
    terminals: t.Tensor,
    gamma: float,
    v_min: float,
    v_max: float,
) -> t.Tensor:
    """Project r + gamma*(1-d)*z onto the fixed support; [B, A] -> [B, A].

    ``2 <= A <= 256``. Positions are computed in fp32 and bin indices
    are clamped to ``[0, A-1]`` (for some supports the fp32 position of
    ``v_max`` rounds to just above ``A-1``), so every row keeps its
    mass.

    Reference semantics: machin/frame/algorithms/rainbow.py:221-301.
    """
    B, A = next_dist.shape
    next_dist = next_dist.detach().float()
    rewards = rewards.detach().float().view(B, 1)
    nd = 1.0 - terminals.detach().float().view(B, 1)
    if next_dist.is_cuda:
        ext = _require_ext()
        return ext.categorical_projection(
            next_dist.contiguous(), rewards.contiguous(), nd.contiguous(),
            float(gamma), float(v_min), float(v_max),
        )
    delta_z = (v_max - v_min) / (A - 1)
    z = t.linspace(v_min, v_max, A, device=next_dist.device)
    tz = (rewards + gamma * nd * z.view(1, A)).clamp(v_min, v_max)
    b = (tz - v_min) / delta_z
    lo_f, hi_f = b.floor(), b.ceil()
    # when b is integral, put all mass on lo
    w_lo = t.where(lo_f == hi_f, t.ones_like(b), hi_f - b)
    w_hi = b - lo_f
    # fp32 (v_max - v_min) / delta_z can round to just above A-1, so
    # the bins are clamped to the support (as in _c51_loss_torch)
    lo = lo_f.long().clamp(0, A - 1)
    hi = hi_f.long().clamp(0, A - 1)
    proj = t.zeros_like(next_dist)
    offset = (t.arange(B, device=next_dist.device) * A).view(B, 1)
    proj.view(-1).index_add_(0, (lo + offset).view(-1), (next_dist * w_lo).view(-1))
    proj.view(-1).index_add_(0, (hi + offset).view(-1), (next_dist * w_hi).view(-1))
    return proj


def _c51_loss_check(dist, action, next_online, next_target, reward,
                    terminal, discount, v_min, v_max):
    """Shared argument validation of :func:`c51_loss`; returns
    ``(action [B], reward [B], terminal [B], discount float or [B])``."""
    if dist.dim() != 3:
        raise ValueError("dist must be [B, A, N]")
    B, A, N = dist.shape
    for name, x in (("next_online", next_online),
                    ("next_target", next_target)):
        if x.shape != dist.shape or x.dtype != dist.dtype:
            raise ValueError(
                f"{name} must have dist's shape and dtype"
            )
    if not 2 <= N <= 256:
        raise ValueError("atoms must be in [2, 256]")
    if not 1 <= A <= 64:
        raise ValueError("actions must be in [1, 64]")
    if not float(v_min) < float(v_max):
        raise ValueError("v_min must be below v_max")
    if action.dtype != t.int64 or action.numel() != B:
        raise ValueError("action must be int64 [B] or [B, 1]")
    if reward.numel() != B or terminal.numel() != B:
        raise ValueError("reward and terminal must have B elements")
    if t.is_tensor(discount):
        if discount.dtype != t.float32 or discount.numel() != B:
            raise ValueError("a tensor discount must be float32 [B]")
        discount = discount.detach().reshape(B)
    else:
        discount = float(discount)
    for name, x in (("action", action), ("next_online", next_online),
                    ("next_target", next_target), ("reward", reward),
                    ("terminal", terminal), ("discount", discount)):
        if t.is_tensor(x) and x.device != dist.device:
            raise ValueError(f"{name} must be on dist's device")
    return (
        action.reshape(B),
        reward.detach().float().reshape(B),
        terminal.detach().float().reshape(B),
        discount,
    )


def _c51_loss_torch(
    dist: t.Tensor, action: t.Tensor, next_online: t.Tensor,
    next_target: t.Tensor, reward: t.Tensor, terminal: t.Tensor,
    discount, v_min: float, v_max: float, from_logits: bool = False,
):
    """Torch composition of :func:`c51_loss` (the CPU path and the
    reference the kernel is tested and timed against). Differentiable
    with respect to ``dist``. Computes in fp32; float64 inputs are
    accepted here (not by the kernel) and computed in float64, for
    gradient checks."""
    if dist.dtype not in (t.float32, t.bfloat16, t.float64):
        raise ValueError("dist must be float32 or bfloat16")
    action, reward, terminal, discount = _c51_loss_check(
        dist, action, next_online, next_target, reward, terminal,
        discount, v_min, v_max,
    )
    B, A, N = dist.shape
    dev = dist.device
    ct = t.float64 if dist.dtype == t.float64 else t.float32
    rows = t.arange(B, device=dev)

    def prob(x):
        x = x.to(ct)
        return t.softmax(x, dim=-1) if from_logits else x

    with t.no_grad():
        v_min, v_max = float(v_min), float(v_max)
        z = t.linspace(v_min, v_max, N, device=dev, dtype=ct)
        q = (prob(next_online) * z.view(1, 1, N)).sum(dim=2)
        best = q.argmax(dim=1)
        nd = prob(next_target)[rows, best]
        if not t.is_tensor(discount):
            discount = t.full((B,), discount, device=dev, dtype=ct)
        gamma = discount.to(device=dev, dtype=ct).view(B, 1)
        alive = 1.0 - terminal.to(ct).view(B, 1)
        delta_z = (v_max - v_min) / (N - 1)
        tz = (reward.to(ct).view(B, 1) + gamma * alive * z.view(1, N)).clamp(
            v_min, v_max
        )
        pos = (tz - v_min) / delta_z
        lo_f, hi_f = pos.floor(), pos.ceil()
        # when pos is integral, all mass goes to lo
        w_lo = t.where(lo_f == hi_f, t.ones_like(pos), hi_f - pos)
        w_hi = pos - lo_f
        lo = lo_f.long().clamp(0, N - 1)
        hi = hi_f.long().clamp(0, N - 1)
        proj = t.zeros_like(nd)
        offset = (rows * N).view(B, 1)
        proj.view(-1).index_add_(0, (lo + offset).view(-1),
                                 (nd * w_lo).view(-1))
        proj.view(-1).index_add_(0, (hi + offset).view(-1),
                                 (nd * w_hi).view(-1))
    pred = dist[rows, action.clamp(0, A - 1)].to(ct)
    if from_logits:
        log_pred = t.log_softmax(pred, dim=-1)
    else:
        log_pred = t.log(pred.clamp_min(1e-8))
    loss = -(proj * log_pred).sum(dim=1)
    return loss, proj, best


class _C51Loss(t.autograd.Function):
    @staticmethod
    def forward(ctx, dist, action, next_online, next_target, reward,
                terminal, discount, v_min, v_max, from_logits):
        ext = _require_ext()
        dist = dist.contiguous()
        tensor_discount = t.is_tensor(discount)
        loss, proj, best, lse, s_sum = ext.c51_loss_fwd(
            dist, action, next_online.contiguous(),
            next_target.contiguous(), reward, terminal,
            discount.contiguous() if tensor_discount else None,
            0.0 if tensor_discount else discount,
            v_min, v_max, from_logits,
        )
        ctx.save_for_backward(dist, action, proj, lse, s_sum)
        ctx.from_logits = from_logits
        ctx.mark_non_differentiable(proj, best)
        return loss, proj, best

    @staticmethod
    def backward(ctx, g_loss, g_proj, g_best):
        dist, action, proj, lse, s_sum = ctx.saved_tensors
        grad = _require_ext().c51_loss_bwd(
            dist, action, proj, lse, s_sum, g_loss.contiguous().float(),
            ctx.from_logits,
        )
        return (grad,) + (None,) * 9


def c51_loss(
    dist: t.Tensor, action: t.Tensor, next_online: t.Tensor,
    next_target: t.Tensor, reward: t.Tensor, terminal: t.Tensor,
    discount, v_min: float, v_max: float, from_logits: bool = False,
):
    """Fused C51 (categorical DQN) loss head with double-DQN action
    selection and a per-sample discount: returns ``(loss [B], proj
    [B, N], best [B])``.

    ``dist``, ``next_online`` and ``next_target`` are ``[B, A, N]``
    (batch, actions, atoms), all fp32 or all bf16: the online net on
    the sampled states, the online net and the target net on the next
    states. ``action`` is int64 ``[B]`` or ``[B, 1]``, ``reward`` and
    ``terminal`` hold ``B`` elements (cast to fp32) and ``discount`` is
    a float or an fp32 ``[B]`` tensor, e.g. ``gamma ** m`` for n-step
    windows of ``m`` steps. Limits: ``2 <= N <= 256``,
    ``1 <= A <= 64``, ``v_min < v_max``.

    With ``dz = (v_max - v_min) / (N - 1)``, ``z_i = v_min + i dz`` and
    ``P(x)`` either ``x`` (``from_logits=False``, the inputs are
    probabilities) or the softmax over atoms (``from_logits=True``),
    all in fp32::

        q[b, a]  = sum_i P(next_online)[b, a, i] z_i
        best[b]  = lowest a with maximal q[b, a]
        nd[b]    = P(next_target)[b, best[b]]
        proj[b]  = nd[b] projected onto the support under
                   tz_i = clamp(reward_b + discount_b (1 - terminal_b) z_i,
                                v_min, v_max)
                   (:func:`categorical_projection` with a per-row
                   discount; bin indices are clamped to [0, N-1])
        a_b      = clamp(action[b], 0, A - 1)
        loss[b]  = -sum_i proj[b, i] log(max(dist[b, a_b, i], 1e-8))
                or -sum_i proj[b, i] log_softmax(dist[b, a_b])_i

    ``loss`` is differentiable with respect to ``dist`` only (``-g proj
    / dist`` where ``dist >= 1e-8``, or ``g (softmax(dist) sum(proj) -
    proj)`` for logits; rows of other actions get zero); ``proj`` and
    ``best`` (int64) are detached.

    On ROCm this is one gfx950 kernel forward and one backward
    (machin_amd/ops/hip/c51_loss.hip); the CPU fallback is the same
    semantics as a torch composition.
    """
    from_logits = bool(from_logits)
    if not dist.is_cuda:
        return _c51_loss_torch(
            dist, action, next_online, next_target, reward, terminal,
            discount, v_min, v_max, from_logits,
        )
    if dist.dtype not in (t.float32, t.bfloat16):
        raise ValueError("dist must be float32 or bfloat16")
    action, reward, terminal, discount = _c51_loss_check(
        dist, action, next_online, next_target, reward, terminal,
        discount, v_min, v_max,
    )
    return _C51Loss.apply(
        dist, action.contiguous(), next_online.detach(),
        next_target.detach(), reward.contiguous(), terminal.contiguous(),
        discount, float(v_min), float(v_max), from_logits,
    )


# ======================================================================
# NoisyLinear (factorised Gaussian noise) and its noise fill
# ======================================================================
# Largest batch (rows of x) the fused kernels take; above it the
# two-GEMM torch form runs on the device. Set from the measured table in
# docs/PERFORMANCE.md ("NoisyLinear").
NOISY_LINEAR_FUSED_MAX_BATCH = 32


def _noisy_linear_check(x, weight_mu, weight_sigma, bias_mu, bias_sigma,
                        eps_in, eps_out, x_dtypes):
    """Shared argument validation of :func:`noisy_linear`; returns
    ``(I, O)``."""
    if x.dtype not in x_dtypes:
        raise ValueError("x must be float32 or bfloat16")
    if weight_mu.dim() != 2:
        raise ValueError("weight_mu must be [O, I]")
    O, I = weight_mu.shape
    if O < 1 or I < 1 or O * I >= 2 ** 31:
        raise ValueError("need I, O >= 1 and O * I < 2^31")
    if x.dim() < 1 or x.shape[-1] != I or x.numel() == 0:
        raise ValueError(f"x must be [..., {I}] and not empty")
    pdt = t.float64 if x.dtype == t.float64 else t.float32
    for name, p, shape in (
        ("weight_mu", weight_mu, (O, I)),
        ("weight_sigma", weight_sigma, (O, I)),
        ("bias_mu", bias_mu, (O,)),
        ("bias_sigma", bias_sigma, (O,)),
        ("eps_in", eps_in, (I,)),
        ("eps_out", eps_out, (O,)),
    ):
        if tuple(p.shape) != shape:
            raise ValueError(f"{name} must have shape {shape}")
        if p.dtype != pdt:
            raise ValueError(f"{name} must be {pdt}")
        if p.device != x.device:
            raise ValueError(f"{name} must be on x's device")
    return I, O


def _noisy_linear_torch(x, weight_mu, weight_sigma, bias_mu, bias_sigma,
                        eps_in, eps_out):
    """Torch composition of :func:`noisy_linear` in the two-GEMM form
    ``x @ mu.T + ((x * eps_in) @ sigma.T) * eps_out + bias`` (the CPU
    path, the device path above the fused batch limit and the reference
    the kernels are timed against). Computes in fp32 and returns x's
    dtype, also inside a ``torch.autocast`` region (autocast is switched
    off for the two GEMMs); float64 inputs are accepted here (not by the
    kernels) and computed in float64, for gradient checks."""
    _noisy_linear_check(
        x, weight_mu, weight_sigma, bias_mu, bias_sigma, eps_in, eps_out,
        (t.float32, t.bfloat16, t.float64),
    )
    ct = t.float64 if x.dtype == t.float64 else t.float32
    eps_in, eps_out = eps_in.detach(), eps_out.detach()
    # inside an autocast region the GEMMs would round x and the weights
    # to bf16; the op computes in fp32 like the kernels
    with t.autocast(device_type=x.device.type, enabled=False):
        xc = x.to(ct)
        y = xc @ weight_mu.t() \
            + ((xc * eps_in) @ weight_sigma.t()) * eps_out
        y = y + (bias_mu + bias_sigma * eps_out)
        return y.to(x.dtype)


class _NoisyLinear(t.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight_mu, weight_sigma, bias_mu, bias_sigma,
                eps_in, eps_out):
        ext = _require_ext()
        x2 = x.reshape(-1, x.shape[-1]).contiguous()
        weight_mu = weight_mu.contiguous()
        weight_sigma = weight_sigma.contiguous()
        eps_in, eps_out = eps_in.contiguous(), eps_out.contiguous()
        y = ext.noisy_linear_fwd(
            x2, weight_mu, weight_sigma, bias_mu.contiguous(),
            bias_sigma.contiguous(), eps_in, eps_out,
        )
        ctx.save_for_backward(x2, weight_mu, weight_sigma, eps_in, eps_out)
        ctx.x_shape = x.shape
        return y.view(*x.shape[:-1], weight_mu.shape[0])

    @staticmethod
    def backward(ctx, g):
        ext = _require_ext()
        x2, weight_mu, weight_sigma, eps_in, eps_out = ctx.saved_tensors
        g2 = g.reshape(-1, weight_mu.shape[0]).to(x2.dtype).contiguous()
        dx = None
        if ctx.needs_input_grad[0]:
            dx = ext.noisy_linear_bwd_input(
                g2, weight_mu, weight_sigma, eps_in, eps_out
            ).view(ctx.x_shape)
        dmu = dsigma = dbias_mu = dbias_sigma = None
        if any(ctx.needs_input_grad[1:5]):
            dmu, dsigma, dbias_mu, dbias_sigma = ext.noisy_linear_bwd_weight(
                g2, x2, eps_in, eps_out
            )
        return dx, dmu, dsigma, dbias_mu, dbias_sigma, None, None


def noisy_linear(x: t.Tensor, weight_mu: t.Tensor, weight_sigma: t.Tensor,
                 bias_mu: t.Tensor, bias_sigma: t.Tensor, eps_in: t.Tensor,
                 eps_out: t.Tensor) -> t.Tensor:
    """Linear layer with factorised Gaussian parameter noise (Fortunato
    et al., "Noisy Networks for Exploration"): returns ``y [..., O]``.

    ``x`` is ``[..., I]`` fp32 or bf16; ``weight_mu`` and
    ``weight_sigma`` are fp32 ``[O, I]``, ``bias_mu``, ``bias_sigma``
    and ``eps_out`` fp32 ``[O]``, ``eps_in`` fp32 ``[I]``;
    ``O * I < 2^31``. All arithmetic is fp32, ``y`` takes ``x``'s dtype
    with one rounding at the store::

        w[o, i] = mu[o, i] + sigma[o, i] * eps_out[o] * eps_in[i]
        y[b, o] = sum_i x[b, i] w[o, i] + bias_mu[o]
                  + bias_sigma[o] * eps_out[o]

    Differentiable in ``x`` and the four parameters (not in the noise)::

        dx[b, i]       = sum_o dy[b, o] w[o, i]
        dmu[o, i]      = sum_b dy[b, o] x[b, i]
        dsigma[o, i]   = dmu[o, i] * eps_out[o] * eps_in[i]
        dbias_mu[o]    = sum_b dy[b, o]
        dbias_sigma[o] = dbias_mu[o] * eps_out[o]

    On ROCm, up to ``NOISY_LINEAR_FUSED_MAX_BATCH`` rows this is one
    gfx950 kernel per line above (machin_amd/ops/hip/noisy_linear.hip):
    ``w`` is never stored, ``mu`` and ``sigma`` are read once forward and
    once for ``dx``, and ``dmu`` / ``dsigma`` come out of one
    accumulator. Sums have a fixed order, so results are reproducible
    bit for bit. Larger batches, and CPU tensors, take the two-GEMM torch
    form ``x @ mu.T + ((x * eps_in) @ sigma.T) * eps_out + bias``.
    """
    if not x.is_cuda:
        return _noisy_linear_torch(
            x, weight_mu, weight_sigma, bias_mu, bias_sigma, eps_in, eps_out
        )
    I, _ = _noisy_linear_check(
        x, weight_mu, weight_sigma, bias_mu, bias_sigma, eps_in, eps_out,
        (t.float32, t.bfloat16),
    )
    if x.numel() // I > NOISY_LINEAR_FUSED_MAX_BATCH:
        return _noisy_linear_torch(
            x, weight_mu, weight_sigma, bias_mu, bias_sigma, eps_in, eps_out
        )
    return _NoisyLinear.apply(
        x, weight_mu, weight_sigma, bias_mu, bias_sigma,
        eps_in.detach(), eps_out.detach(),
    )


def _factorised_noise_torch(buf: t.Tensor, seed: int, offset: int):
    gen = t.Generator(device="cpu")
    gen.manual_seed(
        ((int(seed) * 0x9E3779B97F4A7C15) ^ (int(offset) * 0xD2511F53 + 1))
        & 0x7FFFFFFFFFFFFFFF
    )
    z = t.randn(buf.numel(), generator=gen, dtype=t.float32)
    buf.copy_((z.sign() * z.abs().sqrt()).view_as(buf))
    return buf


def factorised_noise_(buf: t.Tensor, seed: int, offset: int) -> t.Tensor:
    """Fill the contiguous fp32 tensor ``buf`` in place with
    ``f(z) = sign(z) sqrt(|z|)``, ``z ~ N(0, 1)`` (the factorised noise
    of a NoisyLinear layer), and return it.

    On ROCm this is one gfx950 kernel: element ``i`` is drawn from
    Philox keyed by ``(seed, i, offset)``. On CPU the values come from a
    ``torch.Generator`` seeded from ``(seed, offset)``. Each path is
    reproducible for the same ``(seed, offset, buf.numel())``; the CPU
    and the GPU streams do not match each other.
    """
    if buf.dtype != t.float32 or not buf.is_contiguous():
        raise ValueError("buf must be a contiguous float32 tensor")
    seed, offset = int(seed), int(offset)
    if not (0 <= seed < 2 ** 63 and 0 <= offset < 2 ** 63):
        raise ValueError("seed and offset must be in [0, 2^63)")
    if not buf.is_cuda:
        return _factorised_noise_torch(buf, seed, offset)
    if buf.numel():
        _require_ext().factorised_noise_(buf, seed, offset)
    return buf


class _PGHead(t.autograd.Function):
    @staticmethod
    def forward(ctx, logits, actions):
        ext = _require_ext()
        tl, ent = ext.pg_head_fwd(logits.contiguous(),
                                  actions.contiguous())
        ctx.save_for_backward(logits, actions)
        return tl, ent

    @staticmethod
    def backward(ctx, g_taken, g_ent):
        logits, actions = ctx.saved_tensors
        ext = _require_ext()
        d = ext.pg_head_bwd(
            logits.contiguous(), actions.contiguous(),
            g_taken.contiguous().float(), g_ent.contiguous().float(),
        )
        return d, None


def categorical_policy_head(logits: t.Tensor, actions: t.Tensor):
    """Fused categorical policy head: ``(taken_log_prob [N],
    entropy [N])`` from bf16 ``logits [N, A]`` and int64 ``actions
    [N]`` — ONE kernel forward and one backward on ROCm, replacing
    the eager float()->log_softmax->gather->entropy chain (~6+8
    launches of the IMPALA/A2C loss block). Differentiable w.r.t.
    logits (analytic softmax/entropy gradients in the backward
    kernel). CPU fallback uses the identical torch math.
    """
    if logits.is_cuda and logits.dtype == t.bfloat16:
        # the fused kernel consumes bf16 logits (the bench/CNN path);
        # fp32 logits keep the exact eager math below rather than
        # silently quantizing to bf16
        return _PGHead.apply(logits, actions.long().view(-1))
    logp = t.log_softmax(logits.float(), dim=-1)
    tl = logp.gather(
        1, actions.long().view(-1, 1)
    ).view(-1)
    ent = -(logp.exp() * logp).sum(dim=-1)
    return tl, ent


def dequant_u8(frames: t.Tensor, scale: float = 1.0 / 255.0) -> t.Tensor:
    """uint8 -> bf16 with scale, one fused vectorized pass (Atari
    frame normalization; replaces .to(bf16).mul_())."""
    if frames.is_cuda:
        ext = _require_ext()
        out = ext.u8_to_bf16_scale(frames.contiguous().view(-1), scale)
        return out.view(frames.shape)
    return frames.to(t.bfloat16) * scale


def _framestack_gather_torch(
    planes: t.Tensor, base: t.Tensor, k: int, channels_last: bool
):
    """Torch composition of :func:`framestack_gather` (the CPU path
    and the reference the kernel is tested and timed against)."""
    P = planes.shape[0]
    # modular index matrix [B, k+1]; python-style % is non-negative
    idx = (
        base.long().view(-1, 1)
        + t.arange(k + 1, device=base.device).view(1, -1)
    ) % P
    win = planes.index_select(0, idx.view(-1)).view(
        -1, k + 1, *planes.shape[1:]
    )
    fmt = t.channels_last if channels_last else t.contiguous_format
    return (
        win[:, :k].contiguous(memory_format=fmt),
        win[:, 1:].contiguous(memory_format=fmt),
    )


def _framestack_shift_stack(stack: t.Tensor, d: t.Tensor, fmt):
    """``out[b, j, y, x] = stack[b, j, clamp(y + dy_b), clamp(x + dx_b)]``
    with ``d = [B, 2]`` holding ``(dy, dx)``: one advanced-index gather."""
    B, _, H, W = stack.shape
    dev = stack.device
    d = d.long()
    # clamping d first does not change the result (the kernel does it
    # to stay inside int32)
    ys = (t.arange(H, device=dev).view(1, H)
          + d[:, 0:1].clamp(-(H - 1), H - 1)).clamp(0, H - 1)
    xs = (t.arange(W, device=dev).view(1, W)
          + d[:, 1:2].clamp(-(W - 1), W - 1)).clamp(0, W - 1)
    # indexed dims 0, 2, 3 around a slice: the result is [B, H, W, k]
    out = stack[
        t.arange(B, device=dev).view(B, 1, 1), :,
        ys.view(B, H, 1), xs.view(B, 1, W),
    ]
    return out.permute(0, 3, 1, 2).contiguous(memory_format=fmt)


def _framestack_check_shift(shift: t.Tensor, planes: t.Tensor, batch: int):
    if not t.is_tensor(shift) or shift.dtype != t.int32:
        raise ValueError("shift must be an int32 tensor")
    if shift.device != planes.device:
        raise ValueError("shift must be on the device of planes")
    if shift.dim() != 2 or tuple(shift.shape) != (batch, 4):
        raise ValueError("shift must be [B, 4]")
    if not shift.is_contiguous():
        raise ValueError("shift must be contiguous")


def _framestack_gather_shift_torch(
    planes: t.Tensor, base: t.Tensor, k: int, channels_last: bool,
    shift: t.Tensor,
):
    """Torch composition of :func:`framestack_gather` with ``shift``
    (the CPU path and the reference the kernel is tested and timed
    against): the un-shifted composition, then one advanced-index
    gather per stack."""
    state, next_state = _framestack_gather_torch(
        planes, base, k, channels_last
    )
    fmt = t.channels_last if channels_last else t.contiguous_format
    return (
        _framestack_shift_stack(state, shift[:, 0:2], fmt),
        _framestack_shift_stack(next_state, shift[:, 2:4], fmt),
    )


def framestack_gather(
    planes: t.Tensor, base: t.Tensor, k: int, channels_last: bool = False,
    shift: Optional[t.Tensor] = None,
):
    """Rebuild ``(state, next_state)`` frame stacks from a ring of
    frames stored once (frame-deduplicated replay).

    ``planes`` is the u8 ring ``[P, H, W]``, ``base`` int64 ``[B]``.
    Window plane ``j`` (``0 <= j <= k``) of sample ``b`` is ring slot
    ``(base[b] + j) mod P`` (non-negative modulo, so the window may
    wrap and no value of ``base`` addresses outside the ring);
    ``state[b, j]`` is plane ``j`` for ``j < k`` and
    ``next_state[b, j-1]`` is plane ``j`` for ``j >= 1``. Both outputs
    are u8 ``[B, k, H, W]``, plain contiguous or, with
    ``channels_last=True``, in ``torch.channels_last`` strides (memory
    ``[B, H, W, k]``, what the fused u8 conv stem consumes).

    ``shift`` (int32 ``[B, 4]``, contiguous, on the device of
    ``planes``) fuses the random-shift augmentation of DrQ / RAD into
    the gather. Its columns are ``(dy_state, dx_state, dy_next,
    dx_next)``; with ``S`` the stack returned without it::

        out[b, j, y, x] = S[b, j, clamp(y + dy_b, 0, H-1),
                                  clamp(x + dx_b, 0, W-1)]

    one ``(dy, dx)`` for all ``k`` planes of a stack, ``state`` and
    ``next_state`` shifted independently. For ``|d| <= pad`` this is
    "replicate-pad by ``pad``, crop ``H x W`` at ``(pad + dy, pad +
    dx)``"; it is defined for every int32 value (the kernel clamps
    ``dy`` and ``dx`` before adding, which does not change the result).
    ``shift=None`` is the un-shifted code path, call for call.

    On ROCm one gfx950 kernel loads each plane once per sample and
    writes both stacks (machin_amd/ops/hip/framestack.hip); the CPU
    fallback is the same semantics as a torch composition.
    """
    k = int(k)
    if planes.is_cuda:
        ext = _require_ext()
        if shift is not None:
            state, next_state = ext.framestack_gather_shift(
                planes, base, k, bool(channels_last), shift
            )
            return state, next_state
        state, next_state = ext.framestack_gather(
            planes, base, k, bool(channels_last)
        )
        return state, next_state
    if planes.dim() != 3 or planes.dtype != t.uint8:
        raise ValueError("planes must be a uint8 [P, H, W] ring")
    if not 1 <= k <= 8:
        raise ValueError("k must be in [1, 8]")
    if planes.shape[0] < k + 1:
        raise ValueError("ring needs at least k+1 planes")
    if shift is not None:
        _framestack_check_shift(shift, planes, base.numel())
        return _framestack_gather_shift_torch(
            planes, base, k, bool(channels_last), shift
        )
    return _framestack_gather_torch(planes, base, k, bool(channels_last))


def _framestack_gather_nstep_torch(
    planes: t.Tensor, base: t.Tensor, left: t.Tensor, reward: t.Tensor,
    terminal: t.Tensor, pos: t.Tensor, k: int, n: int, gamma: float,
    channels_last: bool,
):
    """Torch composition of :func:`framestack_gather_nstep` (the CPU
    path and the reference the kernel is tested and timed against)."""
    P, T = planes.shape[0], base.shape[0]
    dev = pos.device
    # python-style % is non-negative
    p = pos.long() % T
    s = base.index_select(0, p) % P
    m = left.index_select(0, p).clamp(0, n - 1) + 1
    fmt = t.channels_last if channels_last else t.contiguous_format
    ar_k = t.arange(k, device=dev).view(1, -1)

    def stack(first):
        idx = (first.view(-1, 1) + ar_k) % P
        return planes.index_select(0, idx.view(-1)).view(
            -1, k, *planes.shape[1:]
        ).contiguous(memory_format=fmt)

    ar_n = t.arange(n, device=dev).view(1, -1)
    q = ((p.view(-1, 1) + ar_n) % T).view(-1)
    r = reward.index_select(0, q).view(-1, n)
    d = terminal.index_select(0, q).view(-1, n)
    inside = ar_n < m.view(-1, 1)
    # fp32, in the kernel's order: acc += disc * r; disc *= gamma * (1 - d)
    acc = t.zeros_like(r[:, 0])
    disc = t.ones_like(acc)
    zero = t.zeros_like(acc)
    for j in range(n):
        acc = acc + t.where(inside[:, j], disc * r[:, j], zero)
        disc = disc * (gamma * (1.0 - d[:, j]))
    terminal_n = t.where(
        inside, d, t.full_like(d, float("-inf"))
    ).amax(dim=1)
    return stack(s), stack(s + m), acc, terminal_n, m


def _framestack_gather_nstep_shift_torch(
    planes: t.Tensor, base: t.Tensor, left: t.Tensor, reward: t.Tensor,
    terminal: t.Tensor, pos: t.Tensor, k: int, n: int, gamma: float,
    channels_last: bool, shift: t.Tensor,
):
    """Torch composition of :func:`framestack_gather_nstep` with
    ``shift`` (the CPU path and the reference the kernel is tested and
    timed against): the un-shifted composition, then one advanced-index
    gather per stack. The three scalars are untouched."""
    state, next_state, reward_n, terminal_n, steps = \
        _framestack_gather_nstep_torch(
            planes, base, left, reward, terminal, pos, k, n, gamma,
            channels_last,
        )
    fmt = t.channels_last if channels_last else t.contiguous_format
    return (
        _framestack_shift_stack(state, shift[:, 0:2], fmt),
        _framestack_shift_stack(next_state, shift[:, 2:4], fmt),
        reward_n, terminal_n, steps,
    )


def framestack_gather_nstep(
    planes: t.Tensor, base: t.Tensor, left: t.Tensor, reward: t.Tensor,
    terminal: t.Tensor, pos: t.Tensor, k: int, n: int, gamma: float,
    channels_last: bool = False, shift: Optional[t.Tensor] = None,
):
    """:func:`framestack_gather` with n-step returns computed when
    sampling, from raw 1-step episodes: returns ``(state, next_state,
    reward_n, terminal_n, steps)``.

    ``planes`` is the u8 frame ring ``[P, H, W]``; ``base`` (int64),
    ``left`` (int64), ``reward`` (f32) and ``terminal`` (f32) are the
    WHOLE transition-ring columns ``[T]``, with ``left[p]`` the number
    of transitions that follow ``p`` inside its episode; ``pos`` int64
    ``[B]`` holds the sampled transition-ring positions. Limits:
    ``1 <= k <= 8``, ``1 <= n <= 16``, ``P >= k + n``, ``T >= 1``.

    For sample ``b`` (every modulo non-negative, so no value of
    ``pos``, ``base`` or ``left`` addresses outside either ring)::

        p = pos[b] mod T;  s = base[p] mod P
        m = clamp(left[p], 0, n-1) + 1;  q_j = (p + j) mod T
        reward_n[b]   = sum_{j<m} gamma^j reward[q_j]
                                  prod_{i<j} (1 - terminal[q_i])   (fp32)
        terminal_n[b] = max_{j<m} terminal[q_j]
        steps[b]      = m                                          (int64)
        state[b, j]      = planes[(s + j) mod P]        j < k
        next_state[b, j] = planes[(s + m + j) mod P]    j < k

    ``reward_n`` is the definition of :func:`nstep_returns`; ``m`` does
    not stop early at a terminal (a terminal inside the window only
    sets ``terminal_n``), which is what RAINBOW's host fold stores.
    The stacks are u8 ``[B, k, H, W]``, contiguous or
    ``channels_last``, as in :func:`framestack_gather`; with ``n == 1``
    they are the stacks of ``framestack_gather(planes, base[pos], k)``
    and ``reward_n`` / ``terminal_n`` the stored values.

    ``shift`` (int32 ``[B, 4]``) shifts the two stacks as in
    :func:`framestack_gather`; ``reward_n``, ``terminal_n`` and
    ``steps`` are unaffected, and ``shift=None`` is the un-shifted code
    path, call for call.

    On ROCm the whole op is one gfx950 kernel launch
    (machin_amd/ops/hip/framestack.hip); the CPU fallback is the same
    semantics as a torch composition.
    """
    k, n = int(k), int(n)
    if planes.is_cuda:
        ext = _require_ext()
        if shift is not None:
            return tuple(ext.framestack_gather_nstep_shift(
                planes, base, left, reward, terminal, pos, k, n,
                float(gamma), bool(channels_last), shift,
            ))
        return tuple(ext.framestack_gather_nstep(
            planes, base, left, reward, terminal, pos, k, n, float(gamma),
            bool(channels_last),
        ))
    if planes.dim() != 3 or planes.dtype != t.uint8:
        raise ValueError("planes must be a uint8 [P, H, W] ring")
    if not 1 <= k <= 8:
        raise ValueError("k must be in [1, 8]")
    if not 1 <= n <= 16:
        raise ValueError("n must be in [1, 16]")
    if planes.shape[0] < k + n:
        raise ValueError("ring needs at least k+n planes")
    for name, col, dtype in (
        ("base", base, t.int64), ("left", left, t.int64),
        ("reward", reward, t.float32), ("terminal", terminal, t.float32),
        ("pos", pos, t.int64),
    ):
        if col.dim() != 1 or col.dtype != dtype:
            raise ValueError(f"{name} must be a 1-D {dtype} tensor")
    T = base.shape[0]
    if T < 1 or not left.shape[0] == reward.shape[0] == \
            terminal.shape[0] == T:
        raise ValueError(
            "base, left, reward and terminal must be non-empty columns "
            "of the same length"
        )
    if shift is not None:
        _framestack_check_shift(shift, planes, pos.numel())
        return _framestack_gather_nstep_shift_torch(
            planes, base, left, reward, terminal, pos, k, n, float(gamma),
            bool(channels_last), shift,
        )
    return _framestack_gather_nstep_torch(
        planes, base, left, reward, terminal, pos, k, n, float(gamma),
        bool(channels_last),
    )


# ======================================================================
# per-step vector-env store (machin_amd/ops/hip/framestack_vec.hip)
# ======================================================================
def _framestack_vec_check(planes, reward_col, terminal_col, left, head, run,
                          frame, first, reward, terminal, done, fill, k, n):
    if not 1 <= k <= 8:
        raise ValueError("k must be in [1, 8]")
    if not 1 <= n <= 16:
        raise ValueError("n must be in [1, 16]")
    if not t.is_tensor(planes) or planes.dim() != 3 \
            or planes.dtype != t.uint8 or not planes.is_contiguous():
        raise ValueError("planes must be a contiguous uint8 [E*R, H, W] ring")
    if not t.is_tensor(head) or head.dim() != 1 or head.numel() < 1:
        raise ValueError("head must be [E] with E >= 1")
    E, G = head.numel(), k + n
    H, W = planes.shape[1:]
    if H * W == 0 or planes.shape[0] % E != 0:
        raise ValueError("planes must hold E non-empty rows")
    R = planes.shape[0] // E
    if R - G < 2 * G:
        raise ValueError("lane_slots must be at least 2 * (k + n)")
    for name, v, dtype, shape in (
        ("reward column", reward_col, t.float32, (E * R,)),
        ("terminal column", terminal_col, t.float32, (E * R,)),
        ("left", left, t.int64, (E * R,)),
        ("head", head, t.int64, (E,)),
        ("run", run, t.int64, (E,)),
        ("frame", frame, t.uint8, (E, H, W)),
        ("first", first, t.uint8, (E, k, H, W)),
        ("reward", reward, t.float32, (E,)),
        ("terminal", terminal, t.float32, (E,)),
        ("done", done, t.float32, (E,)),
        ("fill", fill, t.float32, ()),
    ):
        if not t.is_tensor(v) or v.dtype != dtype:
            raise ValueError(f"{name} must be a {dtype} tensor")
        if tuple(v.shape) != shape:
            raise ValueError(
                f"{name} must be {list(shape)}, got {list(v.shape)}"
            )
        if v.device != planes.device:
            raise ValueError(f"{name} must be on the device of planes")
        if name != "first" and not v.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
    if not (first.is_contiguous()
            or first.is_contiguous(memory_format=t.channels_last)):
        raise ValueError(
            "first must be contiguous or in channels_last strides"
        )


def _framestack_vec_append_torch(
    planes: t.Tensor, reward_col: t.Tensor, terminal_col: t.Tensor,
    left: t.Tensor, head: t.Tensor, run: t.Tensor, frame: t.Tensor,
    first: t.Tensor, reward: t.Tensor, terminal: t.Tensor, done: t.Tensor,
    fill: t.Tensor, k: int, n: int,
):
    """Torch composition of :func:`framestack_vec_append` (the CPU path
    and the reference the kernel is tested against). Masked writes use
    boolean indexing, so on a GPU it waits for the device."""
    E, G = head.shape[0], k + n
    R = planes.shape[0] // E
    S = R - G
    dev = planes.device
    lane = t.arange(E, device=dev) * R

    def write(column, slot, value, mask=None):
        """value[e] at slot[e] of lane e's row, and at its mirror."""
        idx = lane + slot
        mirror = slot < G
        if mask is not None:
            idx, value, slot = idx[mask], value[mask], slot[mask]
            mirror = mirror[mask]
        column.index_copy_(0, idx, value)
        column.index_copy_(0, idx[mirror] + S, value[mirror])

    # python-style % is non-negative
    i = head % S
    bs = (i - k) % S
    r = run + 1
    ended = done != 0
    write(planes, i, frame)
    write(reward_col, bs, reward)
    write(terminal_col, bs, terminal)
    write(left, bs, t.zeros_like(i))
    pos = lane + bs

    dead = lane + i
    leaf_idx = dead.view(E, 1).repeat(1, k + 1 + n)
    leaf_w = t.zeros((E, k + 1 + n), dtype=t.float32, device=dev)
    fill = fill.to(t.float32).expand(E)
    zero = t.zeros(E, dtype=t.float32, device=dev)
    for j in range(k):
        slot = (i + 1 + j) % S
        write(planes, slot, first[:, j], ended)
        leaf_idx[:, 1 + j] = t.where(ended, lane + slot, dead)
    for j in range(n):
        # an ended episode: its last min(n, r) windows are complete
        slot = (bs - j) % S
        live = ended & (r > j)
        write(left, slot, t.full_like(i, j), live)
        leaf_idx[:, k + 1 + j] = t.where(live, lane + slot, dead)
        leaf_w[:, k + 1 + j] = t.where(live, fill, zero)
    # a running episode: the step completes the window n - 1 steps back
    slot = (bs - (n - 1)) % S
    live = ~ended & (r >= n)
    write(left, slot, t.full_like(i, n - 1), live)
    leaf_idx[:, k + 1] = t.where(live, lane + slot, leaf_idx[:, k + 1])
    leaf_w[:, k + 1] = t.where(live, fill, leaf_w[:, k + 1])
    head.copy_(t.where(ended, head + 1 + k, head + 1))
    run.copy_(t.where(ended, t.zeros_like(r), r))
    return pos, leaf_idx, leaf_w


def framestack_vec_append(
    planes: t.Tensor, reward_col: t.Tensor, terminal_col: t.Tensor,
    left: t.Tensor, head: t.Tensor, run: t.Tensor, frame: t.Tensor,
    first: t.Tensor, reward: t.Tensor, terminal: t.Tensor, done: t.Tensor,
    fill: t.Tensor, k: int, n: int,
):
    """Store one step of ``E`` envs into the lane rings of
    :class:`~machin_amd.frame.buffers.vec_frame_stack_buffer.DeviceVecFrameStackBuffer`;
    returns ``(pos, leaf_idx, leaf_w)``.

    Layout, with ``G = k + n`` and ``R = S + G``: ``planes`` u8
    ``[E*R, H, W]`` is ``E`` rows of ``S`` ring slots followed by a
    mirror of the row's first ``G`` slots; ``reward_col`` /
    ``terminal_col`` (f32) and ``left`` (int64) are ``[E*R]`` columns
    laid out the same way. "Slot ``i``" below means slot ``i`` of the
    lane's row and, when ``i < G``, also slot ``S + i``. ``head`` and
    ``run`` (int64 ``[E]``) are the planes a lane has written and the
    transitions of its running episode. All six are updated in place.

    Inputs of the step: ``frame`` u8 ``[E, H, W]`` (newest plane of the
    next_state), ``first`` u8 ``[E, k, H, W]`` (contiguous or
    ``channels_last``; the observation after the step, read only for
    lanes whose episode ended), ``reward`` / ``terminal`` / ``done`` f32
    ``[E]`` and ``fill``, a 0-dim f32 tensor. For lane ``e`` with ``i =
    head[e] mod S``, ``bs = (i - k) mod S`` and ``r = run[e] + 1``
    (slots modulo ``S``, non-negative, so no value of ``head``, ``run``
    or ``done`` addresses outside the lane's row)::

        plane i = frame[e]
        reward, terminal, left at bs = reward[e], terminal[e], 0
        pos[e] = e*R + bs;            leaf i -> 0
        if done[e] != 0:
            j < min(n, r):  left at bs-j = j;  leaf bs-j -> fill
            j < k:          plane i+1+j = first[e, j];  leaf i+1+j -> 0
            head[e] += 1 + k;  run[e] = 0
        else:
            r >= n:  left at bs-(n-1) = n-1;  leaf bs-(n-1) -> fill
            head[e] += 1;  run[e] = r

    The leaves are returned, not written: ``leaf_idx`` (int64) and
    ``leaf_w`` (f32) are ``[E, k+1+n]`` with entry 0 the leaf of the
    overwritten plane, entries ``1..k`` the zeroed leaves of an ended
    lane's next first planes, entries ``k+1..k+n`` the filled leaves
    (entry ``k+1+j`` is ``bs-j`` for an ended lane, entry ``k+1`` the
    one filled leaf of a running lane); unused entries repeat ``(e*R +
    i, 0)``, so duplicates carry equal weights and one
    ``DeviceSumTree.update_leaf_batch`` applies the list. ``pos`` is
    the flat position of the step's transition (where its action goes).

    Needs ``S >= 2 * (k + n)``. On ROCm the op is one gfx950 kernel
    launch, one workgroup per lane
    (machin_amd/ops/hip/framestack_vec.hip); the CPU fallback is the
    same semantics as a torch composition.
    """
    k, n = int(k), int(n)
    args = (planes, reward_col, terminal_col, left, head, run, frame, first,
            reward, terminal, done, fill)
    _framestack_vec_check(*args, k, n)
    if planes.is_cuda:
        return tuple(_require_ext().framestack_vec_append(*args, k, n))
    return _framestack_vec_append_torch(*args, k, n)


# ======================================================================
# batched device PixelCatch (machin_amd/ops/hip/pixelcatch.hip)
# ======================================================================
_PC_H = _PC_W = 84
_PC_STATE = 10  # paddle_x ball_x ball_y balls_left steps done hist0..3
_M32 = 0xFFFFFFFF


def _mulhilo32(m: int, x: t.Tensor):
    """(lo, hi) words of ``m * x`` for a 32-bit constant ``m`` and
    int64 tensors holding 32-bit values, without leaving int64."""
    a = m * (x & 0xFFFF)  # < 2^48
    s = m * (x >> 16) + (a >> 16)  # < 2^49
    return ((s & 0xFFFF) << 16) | (a & 0xFFFF), s >> 16


def _philox4x32_10_first(seed: int, offset: t.Tensor, subseq: t.Tensor):
    """Word 0 of Philox4x32-10 with key ``seed`` and counter ``(offset
    lo, offset hi, subseq lo, subseq hi)`` — ``ma_philox4`` of common.h
    as int64 tensor arithmetic."""
    k0, k1 = seed & _M32, (seed >> 32) & _M32
    c0, c1 = offset & _M32, (offset >> 32) & _M32
    c2, c3 = subseq & _M32, (subseq >> 32) & _M32
    for _ in range(10):
        lo0, hi0 = _mulhilo32(0xD2511F53, c0)
        lo1, hi1 = _mulhilo32(0xCD9E8D57, c2)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
    return c0


def _pixelcatch_spawn_x(seed: int, ball_no: t.Tensor) -> t.Tensor:
    env = t.arange(ball_no.shape[0], device=ball_no.device)
    return 3 + _philox4x32_10_first(int(seed), ball_no, env) % 78


def _pixelcatch_pack(px, bx, by):
    return px | (bx << 8) | (by << 16) | (1 << 24)


def _pixelcatch_render(hist: t.Tensor) -> t.Tensor:
    """Packed history entries ``[...]`` -> u8 planes ``[..., 84, 84]``
    (``PixelCatchEnv._frame``; an invalid entry is a zero plane)."""
    h = hist.long()[..., None, None]
    px, bx, by = h & 255, (h >> 8) & 255, (h >> 16) & 255
    valid = ((h >> 24) & 1).bool()
    r = t.arange(_PC_H, device=hist.device).view(_PC_H, 1)
    c = t.arange(_PC_W, device=hist.device).view(1, _PC_W)
    paddle = (r >= _PC_H - 3) & (c >= px - 4) & (c < px + 4)
    ball = (r >= by - 1) & (r <= by + 1) & (c >= bx - 1) & (c <= bx + 1)
    return (valid & (paddle | ball)).to(t.uint8) * 255


def _pixelcatch_check(state, ball_no, obs, others):
    """Shared argument validation of the PixelCatch ops. ``others`` is
    a list of ``(name, tensor, dtype, numel)``."""
    if state.dim() != 2 or state.shape[1] != _PC_STATE \
            or state.dtype != t.int32 or not state.is_contiguous():
        raise ValueError("state must be a contiguous int32 [E, 10] tensor")
    E = state.shape[0]
    if obs.dtype != t.uint8 or tuple(obs.shape) != (E, 4, _PC_H, _PC_W):
        raise ValueError("obs must be uint8 [E, 4, 84, 84]")
    plane = _PC_H * _PC_W
    if obs.stride() not in ((4 * plane, plane, _PC_W, 1),
                            (4 * plane, 1, 4 * _PC_W, 4)):
        raise ValueError(
            "obs must be contiguous or in channels_last strides"
        )
    for name, x, dtype, numel in [("ball_no", ball_no, t.int64, E)] + others:
        if x.dtype != dtype or x.numel() != numel or not x.is_contiguous():
            raise ValueError(
                f"{name} must be a contiguous {dtype} tensor of {numel} "
                f"elements"
            )
    for name, x in [("ball_no", ball_no), ("obs", obs)] + [
        (name, x) for name, x, _, _ in others
    ]:
        if x.device != state.device:
            raise ValueError(f"{name} must be on state's device")


def _pixelcatch_step_check(state, ball_no, action, obs, frame, reward, done,
                           ep_len, balls, max_episode_steps, log):
    E = state.shape[0] if state.dim() == 2 else 0
    others = [
        ("action", action, t.int64, E),
        ("frame", frame, t.uint8, E * _PC_H * _PC_W),
        ("reward", reward, t.float32, E),
        ("done", done, t.float32, E),
        ("ep_len", ep_len, t.int32, E),
    ]
    if log is not None:
        if len(log) != 4:
            raise ValueError(
                "log is (log_frames, log_action, log_reward, log_terminal)"
            )
        frames = log[0]
        if frames.dim() != 4 or frames.shape[0] != E \
                or frames.shape[1] <= 4 \
                or tuple(frames.shape[2:]) != (_PC_H, _PC_W):
            raise ValueError(
                "log_frames must be [E, max_len + 4, 84, 84]"
            )
        max_len = frames.shape[1] - 4
        others += [
            ("log_frames", frames, t.uint8, frames.numel()),
            ("log_action", log[1], t.int64, E * max_len),
            ("log_reward", log[2], t.float32, E * max_len),
            ("log_terminal", log[3], t.float32, E * max_len),
        ]
    _pixelcatch_check(state, ball_no, obs, others)
    if not 1 <= int(balls) <= 2 ** 20:
        raise ValueError("balls must be in [1, 2^20]")
    if not 1 <= int(max_episode_steps) <= 2 ** 30:
        raise ValueError("max_episode_steps must be in [1, 2^30]")


def _pixelcatch_step_torch(
    state: t.Tensor, ball_no: t.Tensor, action: t.Tensor, obs: t.Tensor,
    frame: t.Tensor, reward: t.Tensor, done: t.Tensor, ep_len: t.Tensor,
    seed: int, balls: int, max_episode_steps: int, auto_reset: bool = True,
    log=None,
):
    """Torch composition of :func:`pixelcatch_step` (the CPU path and
    the reference the kernel is tested and timed against; it also runs
    on device tensors, without waiting for the device)."""
    dev = state.device
    E = state.shape[0]
    st = state.long()
    px, bx, by, left, steps, latched = (st[:, i] for i in range(6))
    hist = st[:, 6:]
    no = ball_no.clone()
    env = t.arange(E, device=dev)
    if auto_reset:
        live = t.ones(E, dtype=t.bool, device=dev)
    else:
        live = latched == 0
    act = action.reshape(E).clamp(0, 2)

    px = (px + (act - 1) * 3).clamp(4, _PC_W - 4)
    by = by + 3
    landed = by >= _PC_H - 3
    caught = (bx - px).abs() <= 5
    one = t.ones(E, dtype=t.float32, device=dev)
    rew = t.where(landed, t.where(caught, one, -one), t.zeros_like(one))
    left = left - landed.long()
    dn = landed & (left <= 0)
    spawn = landed & ~dn
    bx = t.where(spawn, _pixelcatch_spawn_x(seed, no), bx)
    by = t.where(spawn, t.zeros_like(by), by)
    no = no + spawn.long()
    length = steps + 1
    dn = dn | (length >= int(max_episode_steps))
    newest = _pixelcatch_pack(px, bx, by)
    pushed = t.cat([hist[:, 1:], newest.view(E, 1)], dim=1)
    new_frame = _pixelcatch_render(newest)
    frame.copy_(t.where(live.view(E, 1, 1), new_frame, frame.view(
        E, _PC_H, _PC_W)).view(frame.shape))

    if log is not None:
        log_frames, log_action, log_reward, log_terminal = log
        max_len = log_frames.shape[1] - 4
        ok = live & (steps >= 0) & (steps < max_len)
        # masked scatter without reading a mask back: rows that do not
        # log rewrite what is there
        col = t.where(ok, steps, t.zeros_like(steps))
        head = log_frames[:, :4]
        head.copy_(t.where((ok & (steps == 0)).view(E, 1, 1, 1),
                           _pixelcatch_render(hist), head))
        log_frames[env, col + 4] = t.where(
            ok.view(E, 1, 1), new_frame, log_frames[env, col + 4]
        )
        for dst, val in (
            (log_action.view(E, max_len), act),
            (log_reward.view(E, max_len), rew),
            (log_terminal.view(E, max_len), dn.float()),
        ):
            dst[env, col] = t.where(ok, val, dst[env, col])

    steps = length
    latched = dn.long()
    if auto_reset:
        fresh = _pixelcatch_spawn_x(seed, no)
        no = no + dn.long()
        px = t.where(dn, t.full_like(px, _PC_W // 2), px)
        bx = t.where(dn, fresh, bx)
        by = t.where(dn, t.zeros_like(by), by)
        left = t.where(dn, t.full_like(left, int(balls)), left)
        steps = t.where(dn, t.zeros_like(steps), steps)
        first = t.zeros_like(pushed)
        first[:, 3] = _pixelcatch_pack(px, bx, by)
        pushed = t.where(dn.view(E, 1), first, pushed)
        latched = t.zeros_like(latched)
    obs.copy_(t.where(live.view(E, 1, 1, 1), _pixelcatch_render(pushed), obs))
    new_state = t.cat(
        [t.stack([px, bx, by, left, steps, latched], dim=1), pushed], dim=1
    )
    state.copy_(t.where(live.view(E, 1), new_state, st))
    ball_no.copy_(t.where(live, no, ball_no))
    reward.copy_(t.where(live, rew, t.zeros_like(rew)).view(reward.shape))
    done.copy_(t.where(live, dn.float(), one).view(done.shape))
    ep_len.copy_(
        t.where(live & dn, length, t.zeros_like(length)).view(ep_len.shape)
    )


def _pixelcatch_reset_torch(state: t.Tensor, ball_no: t.Tensor,
                            mask: t.Tensor, obs: t.Tensor, seed: int,
                            balls: int):
    """Torch composition of :func:`pixelcatch_reset`."""
    E = state.shape[0]
    m = mask.reshape(E) != 0
    st = state.long()
    fresh = t.zeros_like(st)
    fresh[:, 0] = _PC_W // 2
    fresh[:, 1] = _pixelcatch_spawn_x(seed, ball_no)
    fresh[:, 3] = int(balls)
    fresh[:, 9] = _pixelcatch_pack(fresh[:, 0], fresh[:, 1], fresh[:, 2])
    st = t.where(m.view(E, 1), fresh, st)
    state.copy_(st)
    ball_no.add_(m.long())
    obs.copy_(t.where(m.view(E, 1, 1, 1), _pixelcatch_render(st[:, 6:]), obs))


def pixelcatch_step(
    state: t.Tensor, ball_no: t.Tensor, action: t.Tensor, obs: t.Tensor,
    frame: t.Tensor, reward: t.Tensor, done: t.Tensor, ep_len: t.Tensor,
    seed: int, balls: int, max_episode_steps: int, auto_reset: bool = True,
    log=None,
) -> None:
    """Step and render ``E`` PixelCatch envs in place; one env step is
    ``PixelCatchEnv.step`` followed by the optional reset.

    Per-env state (written in place): ``state`` int32 ``[E, 10]`` with
    columns ``paddle_x, ball_x, ball_y, balls_left, steps, done`` and a
    4-entry frame history, newest last, each entry packed as
    ``paddle_x | ball_x << 8 | ball_y << 16 | valid << 24``; ``ball_no``
    int64 ``[E]``, the number of balls the env has ever spawned.
    ``action`` is int64 ``[E]``. Outputs (overwritten): ``obs`` u8
    ``[E, 4, 84, 84]``, plain contiguous or in ``channels_last``
    strides, channel 3 the newest; ``frame`` u8 ``[E, 84, 84]``;
    ``reward`` and ``done`` f32 ``[E]``; ``ep_len`` int32 ``[E]``.

    For env ``e`` (constants of ``pixel_catch.py``)::

        a = clamp(action[e], 0, 2)
        paddle_x = clip(paddle_x + 3 (a - 1), 4, 80);  ball_y += 3
        if ball_y >= 81:
            reward = +1 if |ball_x - paddle_x| <= 5 else -1
            balls_left -= 1
            done if balls_left <= 0, else spawn a ball
        steps += 1;  done if steps >= max_episode_steps
        push (paddle_x, ball_x, ball_y) into the history
        frame[e]  = the newest plane (the terminal frame included)
        ep_len[e] = steps if done else 0
        if done and auto_reset:
            paddle_x = 42, balls_left = balls, steps = 0, spawn a ball,
            history = three invalid (zero) planes + the first frame
        obs[e] = the history, rendered

    The host env raises on an action outside ``{0, 1, 2}``; a kernel
    cannot raise without a sync, so the action is clamped. With
    ``auto_reset=False`` a done env is latched: later steps leave its
    state, ``obs``, ``frame`` and log alone and return reward 0, done 1
    and ``ep_len`` 0 until :func:`pixelcatch_reset`.

    Spawning a ball: ``ball_x = 3 + philox4x32_10(key=seed,
    counter=(ball_no lo, ball_no hi, e lo, e hi))[0] % 78``, then
    ``ball_no += 1`` and ``ball_y = 0``. The range is ``[3, 81)`` as in
    the host env; the modulo bias is 78 / 2^32. The host env's Mersenne
    stream is deliberately not reproduced.

    Rendering is ``PixelCatchEnv._frame``: paddle rows 81..83, columns
    ``[paddle_x - 4, paddle_x + 4)``; ball rows ``[ball_y - 1, ball_y +
    1]`` and columns ``[ball_x - 1, ball_x + 1]``, clipped to the
    screen, value 255, the ball drawn over the paddle.

    ``log = (log_frames [E, max_len + 4, 84, 84] u8, log_action
    [E, max_len] int64, log_reward [E, max_len] f32, log_terminal
    [E, max_len] f32)`` records episodes: the step with in-episode index
    ``s`` (``steps`` before the step, ``s < max_len``) writes ``frame``
    to slot ``4 + s`` and the clamped action, reward and done to column
    ``s``; the step with ``s == 0`` also writes the four planes of the
    episode's first state to slots 0..3 (the reset itself does not, so
    a finished episode's log stays intact until the env's next step).
    Slots ``[0, L + 4)`` are then the ``frames`` of
    ``DeviceFrameStackBuffer.store_frames``.

    On ROCm this is one gfx950 kernel launch on the current stream
    (machin_amd/ops/hip/pixelcatch.hip), a pure write stream of 16-byte
    stores; the CPU fallback is the same semantics as a torch
    composition.
    """
    log = None if log is None else tuple(log)
    _pixelcatch_step_check(state, ball_no, action, obs, frame, reward, done,
                           ep_len, balls, max_episode_steps, log)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    if state.is_cuda:
        ext = _require_ext()
        ext.pixelcatch_step(
            state, ball_no, action, obs, frame, reward, done, ep_len, seed,
            int(balls), int(max_episode_steps), bool(auto_reset),
            *(log if log is not None else (None,) * 4),
        )
        return
    _pixelcatch_step_torch(
        state, ball_no, action, obs, frame, reward, done, ep_len, seed,
        int(balls), int(max_episode_steps), bool(auto_reset), log,
    )


def pixelcatch_reset(state: t.Tensor, ball_no: t.Tensor, mask: t.Tensor,
                     obs: t.Tensor, seed: int, balls: int) -> None:
    """Reset the envs of :func:`pixelcatch_step` whose ``mask`` (u8
    ``[E]``) is non-zero, in place: ``paddle_x = 42``, ``balls_left =
    balls``, ``steps = 0``, ``done = 0``, a new ball, history = three
    invalid entries + the first frame, and ``obs[e]`` = three zero
    planes + that frame (``PixelCatchEnv.reset()``). Other envs and
    every log are left alone."""
    E = state.shape[0] if state.dim() == 2 else 0
    _pixelcatch_check(state, ball_no, obs, [("mask", mask, t.uint8, E)])
    if not 1 <= int(balls) <= 2 ** 20:
        raise ValueError("balls must be in [1, 2^20]")
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    if state.is_cuda:
        _require_ext().pixelcatch_reset(
            state, ball_no, mask, obs, seed, int(balls)
        )
        return
    _pixelcatch_reset_torch(state, ball_no, mask, obs, seed, int(balls))


__all__ = [
    "available",
    "dequant_u8",
    "framestack_gather",
    "framestack_gather_nstep",
    "framestack_vec_append",
    "pixelcatch_step",
    "pixelcatch_reset",
    "polyak_update_",
    "discounted_returns",
    "gae",
    "nstep_returns",
    "vtrace",
    "categorical_projection",
    "categorical_policy_head",
    "c51_loss",
    "noisy_linear",
    "factorised_noise_",
    "FusedPolyak",
    "FusedRMSprop",
]
