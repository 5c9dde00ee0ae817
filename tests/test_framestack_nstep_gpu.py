"""GPU tests for n-step sampling of the frame-deduplicated replay: the
gfx950 ``framestack_gather_nstep`` kernels against the per-sample loop
and against the torch fallback, ``DeviceFrameStackBuffer(n_step=3)`` on
``cuda:0`` against RAINBOW's host fold, and RAINBOW training from it.
u8 stacks, terminals and step counts are compared exactly; rewards
bit-exactly (gamma 0.5, integer rewards) or within
``n * 2^-23 * sum_j gamma^j |r_j|`` of the float64 loop."""
import numpy as np
import pytest
import torch as t

pytestmark = pytest.mark.gpu

if not t.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from machin_amd import ops  # noqa: E402
from machin_amd.frame.buffers import DeviceFrameStackBuffer  # noqa: E402
from util_framestack_nstep import (  # noqa: E402
    N_STEPS, check_op, make_episodes, op_inputs, op_reference, round_trip,
    run_op,
)

DEV = "cuda:0"

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


def _check_against_fallback(got, want, want_loop, kind):
    """Kernel against the CPU fallback: everything exact except the
    reward, where both are within the bound of the float64 loop and so
    within twice the bound of each other."""
    for g, w in zip(got[:2], want[:2]):
        assert g.is_cuda and t.equal(g.cpu(), w)
        # strides of size-1 dims carry no layout information
        assert [s for s, n in zip(g.stride(), g.shape) if n > 1] == [
            s for s, n in zip(w.stride(), w.shape) if n > 1
        ]
    assert t.equal(got[3].cpu(), want[3]) and t.equal(got[4].cpu(), want[4])
    if kind == "exact":
        assert t.equal(got[2].cpu(), want[2])
    else:
        err = (got[2].cpu().double() - want[2].double()).abs()
        assert bool((err <= 2 * want_loop[3]).all())


class TestKernel:
    @pytest.mark.parametrize("kind", ["exact", "random"])
    @pytest.mark.parametrize("n", N_STEPS)
    @pytest.mark.parametrize("h, w, k, channels_last", OP_CASES)
    def test_matches_loop_and_fallback(self, h, w, k, channels_last, n,
                                       kind):
        case = op_inputs(h, w, kind)
        want = op_reference(h, w, kind, k, n)
        got = run_op(ops, case, k, n, channels_last, DEV)
        assert all(out.is_cuda for out in got)
        check_op(got, want, kind, channels_last)
        _check_against_fallback(
            got, run_op(ops, case, k, n, channels_last), want, kind
        )

    @pytest.mark.parametrize("channels_last", [False, True],
                             ids=["nchw", "nhwc"])
    def test_atari_shape(self, channels_last):
        args = (84, 84, "random")
        shape = dict(p_ring=64, t_ring=50, batch=32)
        case = op_inputs(*args, **shape)
        want = op_reference(*args, 4, 3, **shape)
        got = run_op(ops, case, 4, 3, channels_last, DEV)
        check_op(got, want, "random", channels_last)
        _check_against_fallback(
            got, run_op(ops, case, 4, 3, channels_last), want, "random"
        )

    @pytest.mark.parametrize("channels_last", [False, True],
                             ids=["nchw", "nhwc"])
    @pytest.mark.parametrize("h, w, k", [(4, 8, 4), (3, 5, 3)])
    def test_one_step_is_framestack_gather(self, h, w, k, channels_last):
        case = op_inputs(h, w, "random")
        state, next_state, reward, terminal, steps = run_op(
            ops, case, k, 1, channels_last, DEV
        )
        rows = (case.pos % len(case.base)).to(DEV)
        want = ops.framestack_gather(
            case.planes.to(DEV), case.base.to(DEV)[rows], k, channels_last
        )
        assert t.equal(state, want[0]) and t.equal(next_state, want[1])
        assert state.stride() == want[0].stride()
        assert next_state.stride() == want[1].stride()
        assert t.equal(reward, case.reward.to(DEV)[rows])
        assert t.equal(terminal, case.terminal.to(DEV)[rows])
        assert t.equal(steps, t.ones_like(rows))

    def test_rejects_bad_arguments(self):
        c = op_inputs(4, 8, "exact")
        good = dict(planes=c.planes.to(DEV), base=c.base.to(DEV),
                    left=c.left.to(DEV), reward=c.reward.to(DEV),
                    terminal=c.terminal.to(DEV), pos=c.pos.to(DEV),
                    k=4, n=3, gamma=0.5)
        ops.framestack_gather_nstep(**good)
        for bad in (
            dict(n=0), dict(n=17), dict(k=0), dict(k=9),
            dict(planes=good["planes"][:6]),  # P < k + n
            dict(planes=good["planes"].float()),
            dict(planes=good["planes"].view(13, 32)),
            dict(base=good["base"].int()),
            dict(left=good["left"].float()),
            dict(reward=good["reward"].double()),
            dict(terminal=good["terminal"] > 0),
            dict(pos=good["pos"].int()),
            dict(left=good["left"][:5]),
            dict(pos=c.pos),  # host tensor
        ):
            with pytest.raises(RuntimeError):
                ops.framestack_gather_nstep(**{**good, **bad})

    def test_empty_batch(self):
        c = op_inputs(4, 8, "exact")
        out = ops.framestack_gather_nstep(
            c.planes.to(DEV), c.base.to(DEV), c.left.to(DEV),
            c.reward.to(DEV), c.terminal.to(DEV),
            t.empty(0, dtype=t.int64, device=DEV), 4, 3, 0.5,
        )
        assert out[0].shape == out[1].shape == (0, 4, 4, 8)
        assert out[2].shape == out[3].shape == out[4].shape == (0,)


class TestBufferOnDevice:
    def test_wrap_and_eviction_uniform(self):
        buf, batch = round_trip(DEV)
        assert buf._planes.is_cuda and buf._inner.data["_left"].is_cuda
        for part in (batch[0]["state"], batch[3]["state"], batch[2],
                     batch[4], batch[5]["n_step"]):
            assert part.is_cuda
        assert batch[0]["state"].is_contiguous()

    def test_wrap_and_eviction_prioritized(self):
        buf, _ = round_trip(DEV, prioritized=True)
        _, _, idx, weight = buf.sample_batch(16)
        assert idx.is_cuda and weight.is_cuda

    def test_default_is_one_step(self):
        from util_framestack import ATTRS, Episodes

        buf = DeviceFrameStackBuffer(40, DEV)
        buf.store_episode(Episodes().make(5)[0])
        assert "_left" not in buf._inner.data
        n, batch = buf.sample_batch(8, sample_attrs=ATTRS + ["*"])
        assert n == 8 and len(batch) == 6 and batch[5] == {}

    def test_non_float32_reward_raises(self):
        episode = make_episodes([4])[0]
        for tr in episode:
            tr["reward"] = t.tensor([tr["reward"]], dtype=t.float64)
        with pytest.raises(ValueError, match="reward"):
            DeviceFrameStackBuffer(40, DEV, n_step=3).store_episode(episode)


class PixelDistQNet(t.nn.Module):
    """Tiny C51 net on [B, 4, 4, 8] u8 stacks."""

    def __init__(self, action_num=3, atom_num=11):
        super().__init__()
        self.action_num, self.atom_num = action_num, atom_num
        self.fc = t.nn.Linear(4 * 4 * 8, action_num * atom_num)

    def forward(self, state):
        a = self.fc(state.float().flatten(1) / 255.0)
        return t.softmax(a.view(-1, self.action_num, self.atom_num), dim=-1)


class TestRainbowOnDevice:
    def test_ten_updates_nhwc(self):
        from machin_amd.frame.algorithms import RAINBOW

        buf = DeviceFrameStackBuffer(
            200, DEV, n_step=3, discount=0.5, prioritized=True,
            validate=True, frame_layout="nhwc",
        )
        algo = RAINBOW(
            PixelDistQNet().to(DEV), PixelDistQNet().to(DEV), t.optim.Adam,
            -10.0, 10.0, batch_size=16, reward_future_steps=3,
            discount=0.5, replay_buffer=buf,
        )
        for episode in make_episodes([7, 5, 9, 12]):
            algo.store_episode(episode)
        assert buf.size() == 33
        before = buf._tree.weights.clone()
        losses = [algo.update() for _ in range(10)]
        assert all(np.isfinite(v) for v in losses)
        assert buf._tree.weights.is_cuda
        assert not t.equal(buf._tree.weights, before)  # written back
        _, batch, _, _ = buf.sample_batch(
            16, sample_attrs=["next_state", "reward", "*"]
        )
        next_state = batch[0]["state"]
        assert next_state.is_cuda and next_state.shape == (16, 4, 4, 8)
        assert next_state.is_contiguous(memory_format=t.channels_last)
        assert batch[1].is_cuda and batch[2]["n_step"].is_cuda

    def test_mismatched_buffer_raises(self):
        from machin_amd.frame.algorithms import RAINBOW

        algo = RAINBOW(
            PixelDistQNet().to(DEV), PixelDistQNet().to(DEV), t.optim.Adam,
            -10.0, 10.0, batch_size=16, reward_future_steps=3,
            discount=0.5,
            replay_buffer=DeviceFrameStackBuffer(200, DEV, n_step=2,
                                                 discount=0.5),
        )
        with pytest.raises(ValueError, match="reward_future_steps"):
            algo.store_episode(make_episodes([7])[0])
