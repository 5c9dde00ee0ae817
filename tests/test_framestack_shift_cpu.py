"""CPU tests for the random-shift (DrQ) augmentation fused into the
frame-stack gather: the torch fallback of ``shift=`` against a second
formulation (replicate-pad on float, per-sample crop) and
``DeviceFrameStackBuffer(augment_shift=...)``. Everything is compared
exactly."""
import pytest
import torch as t

from machin_amd import ops
from machin_amd.frame.buffers import DeviceFrameStackBuffer
from util_framestack_nstep import op_inputs, run_op
from util_framestack_shift import (
    BASES, INT32_MAX, INT32_MIN, check_buffer, check_strides, pad_crop,
    random_shift, ring,
)

LAYOUTS = pytest.mark.parametrize("channels_last", [False, True],
                                  ids=["nchw", "nhwc"])


class TestOp:
    @pytest.mark.parametrize("pad", [1, 4, 7])
    @pytest.mark.parametrize("k", [1, 4, 8])
    @pytest.mark.parametrize("h, w", [(4, 8), (3, 5), (5, 20), (84, 84)])
    def test_reference_is_pad_and_crop(self, h, w, k, pad):
        planes = ring(11, h, w)
        base = t.tensor([0, 6, 10])
        shift = random_shift(3, pad, seed=h * 100 + k * 10 + pad)
        # the largest offsets in both directions are always present
        shift[0] = t.tensor([pad, -pad, -pad, pad])
        state, next_state = ops._framestack_gather_torch(
            planes, base, k, False
        )
        got = ops._framestack_gather_shift_torch(
            planes, base, k, False, shift
        )
        assert t.equal(got[0], pad_crop(state, shift[:, 0:2], pad))
        assert t.equal(got[1], pad_crop(next_state, shift[:, 2:4], pad))
        via_op = ops.framestack_gather(planes, base, k, shift=shift)
        assert t.equal(via_op[0], got[0]) and t.equal(via_op[1], got[1])

    @LAYOUTS
    def test_zero_and_none_are_unshifted(self, channels_last):
        planes, base = ring(11, 4, 8), t.tensor(BASES)
        want = ops._framestack_gather_torch(planes, base, 4, channels_last)
        zero = t.zeros((len(BASES), 4), dtype=t.int32)
        for shift in (None, zero):
            got = ops.framestack_gather(planes, base, 4, channels_last,
                                        shift=shift)
            for g, w in zip(got, want):
                check_strides(g, w, channels_last)
                assert t.equal(g, w)

    @LAYOUTS
    def test_layout_is_kept(self, channels_last):
        planes, base = ring(11, 4, 8), t.tensor(BASES)
        shift = random_shift(len(BASES), 3)
        plain = ops.framestack_gather(planes, base, 4, False, shift=shift)
        got = ops.framestack_gather(planes, base, 4, channels_last,
                                    shift=shift)
        for g, w in zip(got, plain):
            check_strides(
                g, w.contiguous(memory_format=t.channels_last)
                if channels_last else w, channels_last,
            )
            assert t.equal(g, w)

    def test_int32_extremes(self):
        planes, base = ring(11, 4, 8), t.tensor(BASES)
        shift = t.tensor([[INT32_MAX, INT32_MIN, INT32_MIN, INT32_MAX]],
                         dtype=t.int32).repeat(len(BASES), 1)
        state, next_state = ops._framestack_gather_torch(
            planes, base, 4, False
        )
        got = ops.framestack_gather(planes, base, 4, shift=shift)
        # bottom-left pixel everywhere; top-right for next_state
        assert t.equal(got[0], state[:, :, -1:, :1].expand_as(state))
        assert t.equal(got[1],
                       next_state[:, :, :1, -1:].expand_as(next_state))

    def test_state_and_next_state_use_their_own_columns(self):
        planes, base = ring(11, 4, 8), t.tensor(BASES)
        shift = t.zeros((len(BASES), 4), dtype=t.int32)
        shift[:, 0], shift[:, 1] = 1, -2
        state, next_state = ops._framestack_gather_torch(
            planes, base, 4, False
        )
        got = ops.framestack_gather(planes, base, 4, shift=shift)
        assert t.equal(got[1], next_state)
        assert t.equal(got[0], pad_crop(state, shift[:, 0:2], 2))
        assert not t.equal(got[0], state)

    def test_rejects_bad_shift(self):
        planes, base = ring(11, 4, 8), t.tensor(BASES)
        good = t.zeros((len(BASES), 4), dtype=t.int32)
        for bad in (good.long(), good[:, :2], good[:2],
                    t.zeros((len(BASES), 8), dtype=t.int32)[:, ::2]):
            with pytest.raises(ValueError):
                ops.framestack_gather(planes, base, 4, shift=bad)


class TestNStepOp:
    # m = clamp(left, 0, 2) + 1 covers 1..3: below k = 4, up to and
    # above k = 2
    @LAYOUTS
    @pytest.mark.parametrize("k", [4, 2])
    def test_shifted_stacks_and_untouched_scalars(self, k, channels_last):
        case = op_inputs(4, 8, "exact")
        plain = run_op(ops, case, k, 3, channels_last)
        assert set(plain[4].tolist()) == {1, 2, 3}
        shift = random_shift(len(case.pos), 3, seed=k)
        got = ops.framestack_gather_nstep(
            case.planes, case.base, case.left, case.reward, case.terminal,
            case.pos, k, 3, case.gamma, channels_last=channels_last,
            shift=shift,
        )
        for i, cols in ((0, shift[:, 0:2]), (1, shift[:, 2:4])):
            check_strides(got[i], plain[i], channels_last)
            assert t.equal(got[i], pad_crop(plain[i], cols, 3))
        for i in (2, 3, 4):
            assert t.equal(got[i], plain[i])

    @LAYOUTS
    def test_zero_and_none_are_unshifted(self, channels_last):
        case = op_inputs(4, 8, "exact")
        plain = run_op(ops, case, 4, 3, channels_last)
        zero = t.zeros((len(case.pos), 4), dtype=t.int32)
        for shift in (None, zero):
            got = ops.framestack_gather_nstep(
                case.planes, case.base, case.left, case.reward,
                case.terminal, case.pos, 4, 3, case.gamma,
                channels_last=channels_last, shift=shift,
            )
            for g, w in zip(got[:2], plain[:2]):
                check_strides(g, w, channels_last)
            assert all(t.equal(g, w) for g, w in zip(got, plain))

    def test_int32_extremes_and_own_columns(self):
        case = op_inputs(4, 8, "exact")
        plain = run_op(ops, case, 4, 3, False)
        shift = t.zeros((len(case.pos), 4), dtype=t.int32)
        shift[:, 0], shift[:, 1] = INT32_MAX, INT32_MIN
        got = ops.framestack_gather_nstep(
            case.planes, case.base, case.left, case.reward, case.terminal,
            case.pos, 4, 3, case.gamma, shift=shift,
        )
        assert t.equal(got[0], plain[0][:, :, -1:, :1].expand_as(plain[0]))
        assert t.equal(got[1], plain[1])


class TestBuffer:
    @pytest.mark.parametrize("layout", ["nchw", "nhwc"])
    @pytest.mark.parametrize("n_step", [1, 3])
    def test_off_is_todays_sampling(self, n_step, layout):
        from util_framestack_nstep import ATTRS, make_episodes

        bufs = [
            DeviceFrameStackBuffer(40, "cpu", n_step=n_step, discount=0.5,
                                   frame_layout=layout, **kwargs)
            for kwargs in ({}, {"augment_shift": 0})
        ]
        batches = []
        for buf in bufs:
            for episode in make_episodes([5, 7, 1, 9]):
                buf.store_episode(episode)
            t.manual_seed(7)
            batches.append(buf.sample_batch(32, sample_attrs=ATTRS)[1])
            # the generator is where the other buffer leaves it
            batches.append(t.rand(1))
        (want, want_rand, got, got_rand) = batches
        assert "shift" not in got[5]
        assert set(got[5]) == set(want[5])
        assert t.equal(got[0]["state"], want[0]["state"])
        assert got[0]["state"].stride() == want[0]["state"].stride()
        assert t.equal(got[3]["state"], want[3]["state"])
        assert t.equal(got[2], want[2]) and t.equal(got[4], want[4])
        assert t.equal(got_rand, want_rand)

    @pytest.mark.parametrize("layout", ["nchw", "nhwc"])
    @pytest.mark.parametrize("prioritized", [False, True],
                             ids=["uniform", "per"])
    @pytest.mark.parametrize("n_step", [1, 3])
    def test_on_shifts_the_original_stacks(self, n_step, prioritized,
                                           layout):
        check_buffer("cpu", n_step, prioritized, layout)

    def test_seed_reproduces_the_draw(self):
        buf, first = check_buffer("cpu", 1, False, "nchw")
        t.manual_seed(3)
        again = buf.sample_batch(64, sample_attrs=["*"])[1][0]["shift"]
        assert t.equal(first, again)

    def test_shift_distribution(self):
        from util_framestack import Episodes

        buf = DeviceFrameStackBuffer(40, "cpu", augment_shift=4)
        buf.store_episode(Episodes().make(9)[0])
        t.manual_seed(0)
        shift = buf.sample_batch(4096, sample_attrs=["*"])[1][0]["shift"]
        assert shift.shape == (4096, 4) and shift.dtype == t.int32
        # a value missing from a column: at most 36 * (8/9)^4096
        for col in range(4):
            assert sorted(set(shift[:, col].tolist())) == list(range(-4, 5))
        assert not t.equal(shift[:, 0], shift[:, 2])

    @pytest.mark.parametrize("value", [-1, 17])
    def test_bad_augment_shift_raises(self, value):
        with pytest.raises(ValueError, match="augment_shift"):
            DeviceFrameStackBuffer(40, "cpu", augment_shift=value)

    def test_is_a_named_parameter(self):
        buf = DeviceFrameStackBuffer(40, "cpu", augment_shift=16)
        assert buf.augment_shift == 16
        assert "augment_shift" not in buf._per_kwargs
