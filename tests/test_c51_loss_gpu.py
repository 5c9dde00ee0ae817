"""GPU tests of the fused C51 loss head: the gfx950 ``c51_loss``
kernels against the CPU fallback fed the same values (bf16 inputs
upcast to fp32 for the reference), and the RAINBOW options on
``cuda:0``.

Tolerances: ``rtol=1e-4, atol=1e-3`` (the project's projection
tolerance) for fp32 results; bf16 gradients against the reference
gradient rounded to bf16 with ``rtol=2**-7`` (one bf16 ulp either way)
and ``atol=1e-6``. ``best`` and the zero rows of the gradient are
compared exactly. Rows of ``proj`` sum to the mass of the projected
row within ``1e-5``: 1 for logits and fp32 probabilities; a probability
row stored in bf16 sums to 1 only within ``2^-9``, and the projection
keeps whatever mass it is given.

That ``atol`` is the size of a typical element of ``proj`` and of the
fp32 gradient, so ``TestAgainstHatReference`` holds ``loss``, ``proj``
and the taken row of the gradient, element by element, to the
worst-case fp32 rounding bound derived in
``util_c51_loss.reference_hat`` against its float64 hat-form reference
(a bf16 gradient adds ``2^-8 |ref|``), on every shape and support of
``util_c51_loss.EDGE_CASES``; ``best`` and the rows of untaken actions
are exact. The CPU module checks the bound itself.

MEASURED on one MI355X, the kernels' worst error / bound over all of
``EDGE_CASES``::

    mode    dtype  loss   proj   grad
    prob    fp32   0.092  0.394  0.394
    prob    bf16   0.104  0.394  0.984
    logits  fp32   0.094  0.394  0.392
    logits  bf16   0.087  0.394  0.991

    tie rows (fp32 and bf16)         0.009  0.166  0.96
    scalar discount 0.0, fp32        0.030  0.22   0.22
    scalar discount 1.0, fp32        0.026  0.22   0.22

``proj`` and the fp32 gradients peak on (33, 6, 256) over (-1, 1), the
bf16 gradients and most losses on (8200, 3, 51); the fp32 CPU fallback
reaches 0.39 on the same case as the kernels. ``2^-8`` is the
unit roundoff of bf16 (round to nearest even errs by up to ``2^-8 /
(1 + 2^-8)`` relative), so a bf16 gradient close to 1 is the rounding
of the store among 1.25 million elements, not fp32 error.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch as t
import torch.nn as nn

pytestmark = pytest.mark.gpu

if not t.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from machin_amd import ops  # noqa: E402
from machin_amd.frame.algorithms import RAINBOW  # noqa: E402
from machin_amd.frame.buffers import DeviceFrameStackBuffer  # noqa: E402
from util_c51_loss import (  # noqa: E402
    ALL_SHAPES, ATOL, BACKWARD_SHAPES, EDGE_CASES, RTOL, V_MAX, V_MIN,
    FixedLogitsNet, LogitsQNet, build_rainbow, edge_id, edge_reference,
    expected_logits_loss, fallback_result, make_case, make_edge_case,
    make_tie_case, op_args, pixel_episode, record_update, reference_hat,
    seeded_update, shape_id, taken_rows, worst_ratio,
)

DEV = "cuda:0"
MODES = pytest.mark.parametrize("from_logits", [False, True],
                                ids=["prob", "logits"])
DTYPES = pytest.mark.parametrize("dtype", [t.float32, t.bfloat16],
                                 ids=["fp32", "bf16"])


def close(got, want):
    return t.allclose(got.cpu(), want, rtol=RTOL, atol=ATOL)


class TestForward:
    @MODES
    @DTYPES
    @pytest.mark.parametrize("shape", ALL_SHAPES,
                             ids=[shape_id(s) for s in ALL_SHAPES])
    def test_matches_fallback(self, shape, dtype, from_logits):
        case = make_case(shape, dtype, from_logits)
        want_loss, want_proj, want_best, _ = fallback_result(
            shape, dtype, from_logits
        )
        loss, proj, best = ops.c51_loss(
            *op_args(case, DEV), from_logits=from_logits
        )
        assert loss.is_cuda and proj.is_cuda and best.is_cuda
        assert loss.dtype == proj.dtype == t.float32
        assert best.dtype == t.int64
        assert loss.shape == best.shape == (shape[0],)
        assert proj.shape == (shape[0], shape[2])
        assert t.equal(best.cpu(), want_best)
        assert t.equal(want_best, case.best)
        assert close(proj, want_proj)
        assert close(loss, want_loss)
        # the projection conserves the mass of the row it projects
        row_sum = proj.double().sum(dim=1).cpu()
        nd = case.next_target.double()[t.arange(shape[0]), case.best]
        mass = t.ones(shape[0], dtype=t.float64) if from_logits \
            else nd.sum(dim=1)
        assert float((row_sum - mass).abs().max()) <= 1e-5
        if from_logits or dtype == t.float32:
            # ... which is 1, except for probabilities rounded to bf16,
            # whose rows sum to 1 only within 2^-9
            assert float((row_sum - 1.0).abs().max()) <= 1e-5

    @MODES
    def test_scalar_discount_is_constant_tensor(self, from_logits):
        case = make_case((67, 18, 65), t.float32, from_logits)
        gamma = 0.99 ** 3
        scalar = ops.c51_loss(*op_args(case, DEV, discount=gamma),
                              from_logits=from_logits)
        tensor = ops.c51_loss(
            *op_args(case, DEV,
                     discount=t.full((67,), gamma, device=DEV)),
            from_logits=from_logits,
        )
        for a, b in zip(scalar, tensor):
            assert t.equal(a, b)
        want = ops._c51_loss_torch(*op_args(case, discount=gamma),
                                   from_logits=from_logits)
        assert close(scalar[0], want[0]) and close(scalar[1], want[1])

    def test_terminal_rows_ignore_the_discount(self):
        case = make_case((67, 18, 65), t.float32, True)
        args = list(op_args(case, DEV))
        args[5] = t.ones(67, device=DEV)
        _, proj_a, _ = ops.c51_loss(*args, from_logits=True)
        args[6] = t.rand(67, device=DEV) * 5.0
        _, proj_b, _ = ops.c51_loss(*args, from_logits=True)
        assert t.equal(proj_a, proj_b)
        # all mass on the bin(s) around clamp(reward)
        delta = (V_MAX - V_MIN) / 64
        pos = (case.reward.double().clamp(V_MIN, V_MAX) - V_MIN) / delta
        lo, hi = pos.floor().long(), pos.ceil().long().clamp(max=64)
        proj = proj_a.double().cpu()
        rows = t.arange(67)
        on_bins = proj[rows, lo] + t.where(
            lo == hi, t.zeros_like(pos), proj[rows, hi]
        )
        assert float((on_bins - 1.0).abs().max()) <= 1e-5
        mask = t.ones_like(proj, dtype=t.bool)
        mask[rows, lo] = False
        mask[rows, hi] = False
        assert float(proj[mask].abs().max()) == 0.0
        want_lo = (hi.double() - pos).where(lo != hi, t.ones_like(pos))
        assert t.allclose(proj[rows, lo], want_lo, rtol=RTOL, atol=ATOL)

    @MODES
    def test_out_of_range_action_is_clamped(self, from_logits):
        case = make_case((5, 3, 51), t.float32, from_logits)
        args = list(op_args(case, DEV))
        wild = t.tensor([-3, 3 + 5, 1, -(2 ** 40), 2 ** 40])
        args[0] = args[0].clone().requires_grad_(True)
        args[1] = wild.to(DEV)
        got = ops.c51_loss(*args, from_logits=from_logits)
        (got_grad,) = t.autograd.grad(got[0].sum(), args[0])
        cpu_args = list(op_args(case))
        cpu_args[0] = cpu_args[0].clone().requires_grad_(True)
        cpu_args[1] = wild
        want = ops.c51_loss(*cpu_args, from_logits=from_logits)
        (want_grad,) = t.autograd.grad(want[0].sum(), cpu_args[0])
        assert close(got[0], want[0].detach()) and close(got[1], want[1])
        assert t.equal(got[2].cpu(), want[2])
        assert close(got_grad, want_grad)
        taken = t.zeros(5, 3, dtype=t.bool)
        taken[t.arange(5), wild.clamp(0, 2)] = True
        assert bool((got_grad.cpu()[~taken] == 0).all())

    def test_huge_rewards_land_in_the_edge_bins(self):
        case = make_case((5, 3, 51), t.float32, True)
        args = list(op_args(case, DEV))
        args[4] = t.tensor([1e30, -1e30, 1e30, -1e30, 0.0], device=DEV)
        loss, proj, _ = ops.c51_loss(*args, from_logits=True)
        proj = proj.double().cpu()
        assert bool(t.isfinite(loss).all())
        assert float((proj.sum(dim=1) - 1.0).abs().max()) <= 1e-5
        for row, edge in ((0, 50), (1, 0), (2, 50), (3, 0)):
            assert abs(float(proj[row, edge]) - 1.0) <= 1e-5

    def test_rejects_bad_arguments(self):
        case = make_case((5, 3, 51), t.float32, True)
        good = list(op_args(case, DEV))
        for i, bad in (
            (2, good[2].bfloat16()),
            (3, good[3][:4]),
            (1, good[1][:4]),
            (6, good[6][:4]),
            (0, good[0].double()),
            (4, good[4].cpu()),  # mixed devices
            (1, good[1].cpu()),
            (6, good[6].cpu()),
            (3, good[3].cpu()),
        ):
            args = list(good)
            args[i] = bad
            with pytest.raises(ValueError):
                ops.c51_loss(*args)
        # the binding checks for itself: mixed devices never launch
        from machin_amd.ops import _machin_hip as ext

        with pytest.raises(RuntimeError):
            ext.c51_loss_fwd(
                good[0], good[1], good[2], good[3], good[4].cpu(), good[5],
                None, 0.97, V_MIN, V_MAX, True,
            )
        with pytest.raises(RuntimeError):
            ext.c51_loss_fwd(
                good[0].transpose(0, 1), good[1], good[2], good[3], good[4],
                good[5], None, 0.97, V_MIN, V_MAX, True,
            )


class TestBackward:
    @MODES
    @DTYPES
    @pytest.mark.parametrize("shape", BACKWARD_SHAPES,
                             ids=[shape_id(s) for s in BACKWARD_SHAPES])
    def test_matches_autograd_of_fallback(self, shape, dtype, from_logits):
        case = make_case(shape, dtype, from_logits)
        want = fallback_result(shape, dtype, from_logits)[3]
        args = list(op_args(case, DEV))
        args[0] = args[0].clone().requires_grad_(True)
        loss, _, _ = ops.c51_loss(*args, from_logits=from_logits)
        (grad,) = t.autograd.grad(loss, args[0], case.g.to(DEV))
        assert grad.dtype == dtype and grad.shape == args[0].shape
        grad = grad.cpu()
        B, A, _ = shape
        taken = t.zeros(B, A, dtype=t.bool)
        taken[t.arange(B), case.action] = True
        assert bool((grad[~taken] == 0).all())
        assert bool((want[~taken] == 0).all())
        if dtype == t.float32:
            assert t.allclose(grad, want, rtol=RTOL, atol=ATOL)
        else:
            assert t.allclose(grad.float(), want.bfloat16().float(),
                              rtol=2.0 ** -7, atol=1e-6)

    @DTYPES
    def test_clamp_mask(self, dtype):
        case = make_case((5, 3, 51), dtype, False)
        args = list(op_args(case, DEV))
        dist = args[0].clone()
        rows = t.arange(5, device=DEV)
        act = case.action.to(DEV)
        dist[rows, act, 0] = 0.0
        dist[rows, act, 7] = 1e-9
        dist[rows[:2], act[:2], 50] = 0.0
        args[0] = dist.requires_grad_(True)
        loss, proj, _ = ops.c51_loss(*args, from_logits=False)
        assert bool(t.isfinite(loss).all())
        (grad,) = t.autograd.grad(loss, args[0], case.g.to(DEV))
        assert bool(t.isfinite(grad).all())
        assert bool((grad[rows, act, 0] == 0).all())
        assert bool((grad[rows, act, 7] == 0).all())
        assert bool((grad[rows[:2], act[:2], 50] == 0).all())
        # the others keep -g * proj / dist
        want = -case.g.to(DEV) * proj[:, 3] / dist[rows, act, 3].float()
        got = grad[rows, act, 3].float()
        if dtype == t.float32:
            assert t.allclose(got, want, rtol=RTOL, atol=ATOL)
        else:
            assert t.allclose(got, want.bfloat16().float(),
                              rtol=2.0 ** -7, atol=1e-6)


# -- the kernels against the hat-form reference and its bound --------------
def run_device(case, discount=None):
    """Forward and backward of the kernels on a case: ``(loss, proj,
    best, grad [B, A, N])`` on the device."""
    args = list(op_args(case, DEV, discount=discount))
    args[0] = args[0].clone().requires_grad_(True)
    loss, proj, best = ops.c51_loss(*args, from_logits=case.from_logits)
    (grad,) = t.autograd.grad(loss, args[0], case.g.to(DEV))
    return loss.detach(), proj, best, grad


def within_bound(case, result, what, shared=True):
    """Every output of ``result`` against the hat-form reference of a
    case (the shared one of an unmodified edge case) and its bound;
    prints the worst error/bound of each."""
    ref, bound = edge_reference(
        (case.shape, case.v_min, case.v_max), case.dtype, case.from_logits
    ) if shared else reference_hat(case)
    loss, proj, best, grad = (x.cpu() for x in result)
    assert grad.dtype == case.dtype and grad.shape == case.dist.shape
    assert loss.dtype == proj.dtype == t.float32
    rows, others_zero = taken_rows(grad, case)
    ok = others_zero and t.equal(best, ref.best)
    for name, got in (("loss", loss), ("proj", proj), ("grad", rows)):
        ratio, inside = worst_ratio(got, getattr(ref, name),
                                    getattr(bound, name))
        print(f"{what} {name} worst error/bound {ratio:.3g}")
        ok = ok and inside
    # the projection conserves the mass of the row it projects
    nd = case.next_target.double()[t.arange(case.shape[0]), ref.best]
    mass = t.ones(case.shape[0], dtype=t.float64) if case.from_logits \
        else nd.sum(dim=1)
    conserved = float((proj.double().sum(dim=1) - mass).abs().max()) <= 1e-5
    return ok and conserved


def with_discount(case, value):
    """A copy of a case with every discount set to ``value``."""
    copy = SimpleNamespace(**vars(case))
    copy.discount = t.full_like(case.discount, value)
    return copy


class TestAgainstHatReference:
    @MODES
    @DTYPES
    @pytest.mark.parametrize("case_key", EDGE_CASES,
                             ids=[edge_id(c) for c in EDGE_CASES])
    def test_within_the_bound(self, case_key, dtype, from_logits):
        case = make_edge_case(*case_key, dtype, from_logits)
        mode = "logits" if from_logits else "prob"
        name = "bf16" if dtype == t.bfloat16 else "fp32"
        assert within_bound(case, run_device(case),
                            f"{mode} {name} {edge_id(case_key)}")

    @MODES
    @DTYPES
    def test_tie_goes_to_the_lower_action(self, dtype, from_logits):
        case = make_tie_case(dtype, from_logits)
        result = run_device(case)
        assert t.equal(result[2].cpu(), case.best)
        assert within_bound(case, result, "tie", shared=False)

    @MODES
    @pytest.mark.parametrize("gamma", [0.0, 1.0])
    def test_scalar_discounts_zero_and_one(self, gamma, from_logits):
        case = with_discount(
            make_edge_case((67, 18, 65), V_MIN, V_MAX, t.float32,
                           from_logits), gamma)
        scalar = run_device(case, discount=gamma)
        tensor = run_device(case)
        for a, b in zip(scalar, tensor):
            assert t.equal(a, b)
        assert within_bound(case, scalar, f"scalar discount {gamma:g}",
                            shared=False)

    @MODES
    @pytest.mark.parametrize("where", ["reward", "next_target", "dist"])
    def test_nan_stays_in_its_row(self, where, from_logits):
        """Nine rows are three blocks of four waves that share one LDS
        array: row 5 sits between rows 4, 6 and 7 of its block. Only
        values are poisoned; every index the kernels form is clamped
        (NaN positions go through fminf/fmaxf to bin 0, actions and
        ``best`` are clamped), so no address depends on the NaN."""
        src = make_edge_case((9, 4, 124), V_MIN, V_MAX, t.float32,
                             from_logits)
        b = 5
        case = SimpleNamespace(**vars(src))
        nan = float("nan")
        if where == "reward":
            case.reward = src.reward.clone()
            case.reward[b] = nan
        elif where == "next_target":
            case.next_target = src.next_target.clone()
            case.next_target[b, int(src.best[b]), 3] = nan
        else:
            case.dist = src.dist.clone()
            case.dist[b, int(src.action[b]), 3] = nan
        clean, dirty = run_device(src), run_device(case)
        assert bool(t.isnan(dirty[0][b]))
        others = t.tensor([i for i in range(9) if i != b], device=DEV)
        for a, d in zip(clean, dirty):
            assert t.equal(a[others], d[others])
        assert not bool(t.isnan(clean[0]).any())


# -- RAINBOW on the device -------------------------------------------------
class PixelLogitsQNet(nn.Module):
    """Tiny conv + MLP C51 net on [B, 4, 16, 16] u8 stacks; logits."""

    def __init__(self, action_num=3, atom_num=11):
        super().__init__()
        self.action_num, self.atom_num = action_num, atom_num
        self.conv = nn.Conv2d(4, 4, 4, stride=4)
        self.fc = nn.Linear(4 * 4 * 4, action_num * atom_num)

    def forward(self, state):
        a = t.relu(self.conv(state.float() / 255.0)).flatten(1)
        return self.fc(a).view(-1, self.action_num, self.atom_num)


class TestRainbowOnDevice:
    def test_same_step_as_eager(self):
        eager = build_rainbow(DEV)
        fused = build_rainbow(DEV, fused_loss=True)
        before = [p.detach().clone() for p in fused.qnet.parameters()]
        loss_eager, loss_fused = seeded_update(eager), seeded_update(fused)
        assert np.isfinite(loss_eager)
        assert loss_fused == pytest.approx(loss_eager, rel=RTOL, abs=ATOL)
        for p, q, p0 in zip(eager.qnet.parameters(),
                            fused.qnet.parameters(), before):
            assert q.is_cuda and not t.equal(q, p0)
            assert t.allclose(p, q, rtol=RTOL, atol=ATOL)

    def test_logits_mlp_updates(self, monkeypatch):
        """The logits reach the kernel as logits, and the returned loss
        is the IS-weighted mean of -sum(proj * log_softmax), recomputed
        in float64 on the CPU from the tensors that reached the op."""
        algo = build_rainbow(DEV, net=LogitsQNet, fused_loss=True,
                             dist_from_logits=True)
        calls = record_update(monkeypatch, algo)
        before = [p.detach().clone() for p in algo.qnet.parameters()]
        loss = seeded_update(algo)
        (call,) = calls
        assert call.kwargs["from_logits"] is True
        assert all(x.is_cuda for x in call.args[:6])
        row_sums = call.args[0].detach().sum(dim=-1)
        assert float((row_sums - 1.0).abs().min()) > 1e-3
        assert np.isfinite(loss)
        assert loss == pytest.approx(expected_logits_loss(call),
                                     rel=RTOL, abs=ATOL)
        assert all(not t.equal(p, p0)
                   for p, p0 in zip(algo.qnet.parameters(), before))

    def test_logits_model_acts_on_softmaxed_values(self):
        algo = RAINBOW(
            FixedLogitsNet().to(DEV), FixedLogitsNet().to(DEV),
            t.optim.Adam, V_MIN, V_MAX, fused_loss=True,
            dist_from_logits=True,
        )
        state = {"state": t.rand(5, 4, device=DEV)}
        # greedy on the raw logits would be action 1 (see FixedLogitsNet)
        assert algo.act_discrete(state).view(-1).tolist() == [0] * 5

    def test_all_options_on_framestack_replay(self, monkeypatch):
        buf = DeviceFrameStackBuffer(
            200, DEV, n_step=3, discount=0.9, prioritized=True
        )
        algo = RAINBOW(
            PixelLogitsQNet().to(DEV), PixelLogitsQNet().to(DEV),
            t.optim.Adam, V_MIN, V_MAX, batch_size=8,
            reward_future_steps=3, discount=0.9, replay_buffer=buf,
            fused_loss=True, exact_nstep_bootstrap=True,
            dist_from_logits=True,
        )
        for seed, length in enumerate((7, 5, 9)):
            algo.store_episode(pixel_episode(length, 16, 16, seed=seed))
        calls = record_update(monkeypatch, algo)
        every = t.arange(buf._t_capacity, device=DEV)
        before = buf._tree.get_leaf_weight(every).clone()
        loss = algo.update()
        assert np.isfinite(loss)
        (call,) = calls
        index = call.index
        assert index.is_cuda and index.shape == (8,)
        # logits in, as logits; per-sample discount 0.9 ** m on the device
        assert call.kwargs["from_logits"] is True
        discount = call.args[6]
        assert t.is_tensor(discount) and discount.is_cuda
        assert discount.dtype == t.float32 and discount.shape == (8,)
        assert set(discount.cpu().double().mul(1000).round().tolist()) <= {
            900.0, 810.0, 729.0
        }
        assert loss == pytest.approx(expected_logits_loss(call),
                                     rel=RTOL, abs=ATOL)
        after = buf._tree.get_leaf_weight(every)
        assert after.is_cuda
        assert bool((after[index] != before[index]).all())
