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
"""
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
    ALL_SHAPES, ATOL, BACKWARD_SHAPES, RTOL, V_MAX, V_MIN, FixedLogitsNet,
    LogitsQNet, build_rainbow, expected_logits_loss, fallback_result,
    make_case, op_args, pixel_episode, record_update, seeded_update,
    shape_id,
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
