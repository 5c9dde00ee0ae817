"""N-step sampling of the frame-deduplicated replay on the CPU fallback
path: ``ops.framestack_gather_nstep`` against the per-sample loop,
``DeviceFrameStackBuffer(n_step=3)`` against RAINBOW's host fold, and
RAINBOW storing raw episodes into it. u8 stacks, terminals and step
counts are compared exactly; rewards bit-exactly (gamma 0.5, integer
rewards) or within ``n * 2^-23 * sum_j gamma^j |r_j|`` (2n roundings of
relative size 2^-24; covers FMA contraction and either summation
order)."""
import numpy as np
import pytest
import torch as t

from machin_amd import ops
from machin_amd.frame.buffers import DeviceFrameStackBuffer
from util_framestack import Episodes
from util_framestack import ATTRS as ATTRS_1STEP
from util_framestack_nstep import (
    N_STEPS, check_op, make_episodes, op_inputs, op_reference, round_trip,
    run_op,
)

# (H, W, k, layouts): vector path, scalar path, NHWC with k != 4
SHAPES = [
    (4, 8, 4, (False, True)),
    (3, 5, 3, (False, True)),
    (4, 8, 3, (True,)),
]
OP_CASES = [
    pytest.param(h, w, k, cl, id=f"{h}x{w}-k{k}-{'nhwc' if cl else 'nchw'}")
    for h, w, k, layouts in SHAPES for cl in layouts
]


class TestOpFallback:
    @pytest.mark.parametrize("kind", ["exact", "random"])
    @pytest.mark.parametrize("n", N_STEPS)
    @pytest.mark.parametrize("h, w, k, channels_last", OP_CASES)
    def test_matches_loop(self, h, w, k, channels_last, n, kind):
        case = op_inputs(h, w, kind)
        got = run_op(ops, case, k, n, channels_last)
        check_op(got, op_reference(h, w, kind, k, n), kind, channels_last)

    @pytest.mark.parametrize("channels_last", [False, True])
    def test_one_step_is_framestack_gather(self, channels_last):
        case = op_inputs(4, 8, "random")
        state, next_state, reward, terminal, steps = run_op(
            ops, case, 4, 1, channels_last
        )
        rows = case.pos % len(case.base)
        want = ops.framestack_gather(
            case.planes, case.base[rows], 4, channels_last
        )
        assert t.equal(state, want[0]) and t.equal(next_state, want[1])
        assert state.stride() == want[0].stride()
        assert next_state.stride() == want[1].stride()
        assert t.equal(reward, case.reward[rows])
        assert t.equal(terminal, case.terminal[rows])
        assert t.equal(steps, t.ones_like(rows))

    def test_rejects_bad_arguments(self):
        c = op_inputs(4, 8, "exact")
        good = dict(planes=c.planes, base=c.base, left=c.left,
                    reward=c.reward, terminal=c.terminal, pos=c.pos,
                    k=4, n=3, gamma=0.5)
        ops.framestack_gather_nstep(**good)
        for bad in (
            dict(n=0), dict(n=17), dict(k=0), dict(k=9),
            dict(planes=c.planes[:6]),  # P < k + n
            dict(planes=c.planes.float()),
            dict(planes=c.planes.view(13, 32)),
            dict(base=c.base.int()), dict(left=c.left.float()),
            dict(reward=c.reward.double()),
            dict(terminal=c.terminal > 0), dict(pos=c.pos.int()),
            dict(left=c.left[:5]),
        ):
            with pytest.raises(ValueError):
                ops.framestack_gather_nstep(**{**good, **bad})

    def test_exported(self):
        assert "framestack_gather_nstep" in ops.__all__


class TestBufferNStep:
    def test_wrap_and_eviction_uniform(self):
        round_trip("cpu")

    def test_wrap_and_eviction_prioritized(self):
        buf, _ = round_trip("cpu", prioritized=True)
        _, _, idx, weight = buf.sample_batch(16)
        assert idx.shape == weight.shape == (16,)

    def test_nhwc_layout(self):
        _, batch = round_trip("cpu", stores=6, frame_layout="nhwc")
        for stack in (batch[0]["state"], batch[3]["state"]):
            assert stack.is_contiguous(memory_format=t.channels_last)

    def test_hidden_columns_never_leak(self):
        buf, _ = round_trip("cpu", stores=3)
        assert {"_base", "_left"} <= set(buf._inner.data)
        _, batch = buf.sample_batch(8)  # default attrs
        names = set()
        for part in batch:
            assert isinstance(part, dict) or t.is_tensor(part)
            if isinstance(part, dict):
                names |= set(part)
        assert not {"_base", "_left"} & names
        assert set(batch[-1]) == {"n_step"}

    def test_default_is_one_step(self):
        """n_step=1: same tuple structure as before, no n_step
        attribute under "*", no extra column."""
        buf = DeviceFrameStackBuffer(40, "cpu")
        assert buf.n_step == 1 and buf.discount == 0.99
        episode, _ = Episodes().make(5)
        buf.store_episode(episode)
        assert "_left" not in buf._inner.data
        n, batch = buf.sample_batch(8, sample_attrs=ATTRS_1STEP + ["*"])
        assert n == 8 and len(batch) == 6
        assert batch[5] == {}
        n, batch = buf.sample_batch(8)
        assert [type(part) for part in batch] == [dict, dict, t.Tensor,
                                                  dict, t.Tensor, dict]
        assert batch[5] == {}

    def test_constructor_arguments(self):
        buf = DeviceFrameStackBuffer(40, "cpu", n_step=3, discount=0.5)
        assert buf.n_step == 3 and buf.discount == 0.5
        for bad in (0, 17, -1):
            with pytest.raises(ValueError):
                DeviceFrameStackBuffer(40, "cpu", n_step=bad)
        with pytest.raises(ValueError):
            DeviceFrameStackBuffer(6, "cpu", n_step=3)  # < k + n

    @pytest.mark.parametrize("column", ["reward", "terminal"])
    def test_non_float32_column_raises(self, column):
        episode = make_episodes([4])[0]
        for tr in episode:
            tr[column] = t.tensor([float(tr[column])], dtype=t.float64)
        with pytest.raises(ValueError, match=column):
            DeviceFrameStackBuffer(40, "cpu", n_step=3).store_episode(
                episode
            )
        # the 1-step buffer keeps accepting such columns
        DeviceFrameStackBuffer(40, "cpu").store_episode(episode)


class PixelDistQNet(t.nn.Module):
    """Tiny C51 net on [B, 4, 4, 8] u8 stacks."""

    def __init__(self, action_num=3, atom_num=11):
        super().__init__()
        self.action_num, self.atom_num = action_num, atom_num
        self.fc = t.nn.Linear(4 * 4 * 8, action_num * atom_num)

    def forward(self, state):
        a = self.fc(state.float().flatten(1) / 255.0)
        return t.softmax(a.view(-1, self.action_num, self.atom_num), dim=-1)


def _rainbow(buffer, n=3, gamma=0.5):
    from machin_amd.frame.algorithms import RAINBOW

    return RAINBOW(
        PixelDistQNet(), PixelDistQNet(), t.optim.Adam, -10.0, 10.0,
        batch_size=16, reward_future_steps=n, discount=gamma,
        replay_buffer=buffer,
    )


class TestRainbowOnNStepReplay:
    def test_stores_raw_episodes_and_updates(self):
        buf = DeviceFrameStackBuffer(
            200, "cpu", n_step=3, discount=0.5, prioritized=True,
            validate=True,
        )
        algo = _rainbow(buf)
        episodes = make_episodes([7, 5, 9])
        for episode in episodes:
            algo.store_episode(episode)
        assert buf.size() == 21
        # raw 1-step rewards were stored, not folded ones
        stored = buf._inner.data["reward"][:7].tolist()
        assert stored == [tr["reward"] for tr in episodes[0]]
        losses = [algo.update() for _ in range(3)]
        assert all(np.isfinite(v) for v in losses)

    def test_mismatched_buffer_raises(self):
        episode = make_episodes([7])[0]
        for kwargs in (dict(n_step=2, discount=0.5),
                       dict(n_step=3, discount=0.9)):
            algo = _rainbow(DeviceFrameStackBuffer(200, "cpu", **kwargs))
            with pytest.raises(ValueError, match="reward_future_steps"):
                algo.store_episode(episode)
            assert algo.replay_buffer.size() == 0
