"""GPU tests for frame-deduplicated replay: the gfx950
``framestack_gather`` kernel against the torch fallback (exact), the
``DeviceFrameStackBuffer`` on ``cuda:0`` and its use from DQN / DQNPer
and the fused u8 conv stem."""
import numpy as np
import pytest
import torch as t
import torch.nn as nn

pytestmark = pytest.mark.gpu

if not t.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from machin_amd import ops  # noqa: E402
from machin_amd.frame.buffers import DeviceFrameStackBuffer  # noqa: E402
from util_framestack import round_trip  # noqa: E402

DEV = "cuda:0"
BASES = [0, 3, 6, 7, 10, 10]


def _ring(p, h, w, seed=0):
    gen = t.Generator().manual_seed(seed)
    return t.randint(0, 256, (p, h, w), dtype=t.uint8, generator=gen)


def _check(ring, base, k, channels_last, ring_dev=None):
    """Kernel output == CPU fallback output, byte for byte."""
    base = t.as_tensor(base, dtype=t.int64)
    want = ops.framestack_gather(ring, base, k, channels_last)
    ring_dev = ring.to(DEV) if ring_dev is None else ring_dev
    got = ops.framestack_gather(ring_dev, base.to(DEV), k, channels_last)
    for g, w in zip(got, want):
        assert g.is_cuda and g.dtype == t.uint8 and g.shape == w.shape
        # strides of size-1 dims carry no layout information
        assert [s for s, n in zip(g.stride(), g.shape) if n > 1] == [
            s for s, n in zip(w.stride(), w.shape) if n > 1
        ]
        if channels_last:
            assert g.is_contiguous(memory_format=t.channels_last)
        else:
            assert g.is_contiguous()
        assert t.equal(g.cpu(), w)


@pytest.mark.parametrize("channels_last", [False, True],
                         ids=["nchw", "nhwc"])
class TestKernelMatchesFallback:
    def test_vector_path_two_chunks(self, channels_last):
        _check(_ring(11, 4, 8), BASES, 4, channels_last)

    def test_scalar_path(self, channels_last):
        _check(_ring(11, 3, 5), BASES, 4, channels_last)

    @pytest.mark.parametrize("k", [1, 2, 8])
    def test_other_stack_depths(self, channels_last, k):
        # NHWC with k != 4 is the generic interleave
        _check(_ring(11, 4, 8), BASES, k, channels_last)

    def test_atari_small_batch(self, channels_last):
        _check(_ring(64, 84, 84), [0, 61, 63], 4, channels_last)

    def test_atari_grid_stride(self, channels_last):
        # 1200 * 441 work items > 2048 blocks * 256 threads
        gen = t.Generator().manual_seed(5)
        base = t.randint(0, 64, (1200,), generator=gen)
        _check(_ring(64, 84, 84), base, 4, channels_last)

    def test_out_of_range_base(self, channels_last):
        p = 11
        _check(_ring(p, 4, 8), [-1, p + 2, -p, -(2 ** 40), 2 ** 62],
               4, channels_last)

    def test_unaligned_ring_takes_scalar_path(self, channels_last):
        ring = _ring(11, 4, 8)
        flat = t.empty(11 * 32 + 1, dtype=t.uint8, device=DEV)
        view = flat[1:].view(11, 4, 8)
        view.copy_(ring)
        assert view.data_ptr() % 16 != 0
        _check(ring, BASES, 4, channels_last, ring_dev=view)

    def test_side_stream(self, channels_last):
        ring = _ring(64, 84, 84)
        base = t.tensor([5, 62, 0, 33])
        want = ops.framestack_gather(ring, base, 4, channels_last)
        ring_dev, base_dev = ring.to(DEV), base.to(DEV)
        side = t.cuda.Stream()
        side.wait_stream(t.cuda.current_stream())
        with t.cuda.stream(side):
            got = ops.framestack_gather(ring_dev, base_dev, 4,
                                        channels_last)
        side.synchronize()
        assert t.equal(got[0].cpu(), want[0])
        assert t.equal(got[1].cpu(), want[1])


class TestBindingChecks:
    def test_rejects_bad_arguments(self):
        ring = _ring(11, 4, 8).to(DEV)
        base = t.tensor([0], device=DEV)
        ext = ops._require_ext()
        with pytest.raises(RuntimeError):
            ext.framestack_gather(ring, base, 0, False)
        with pytest.raises(RuntimeError):
            ext.framestack_gather(ring, base, 9, False)
        with pytest.raises(RuntimeError):
            ext.framestack_gather(ring[:4], base, 4, False)  # P < k+1
        with pytest.raises(RuntimeError):
            ext.framestack_gather(ring.view(11, 32), base, 4, False)
        with pytest.raises(RuntimeError):
            ext.framestack_gather(ring.float(), base, 4, False)
        with pytest.raises(RuntimeError):
            ext.framestack_gather(ring, base.int(), 4, False)
        with pytest.raises(RuntimeError):
            ext.framestack_gather(ring, base.cpu(), 4, False)
        with pytest.raises(RuntimeError):
            ext.framestack_gather(ring[:, :, ::2], base, 4, False)

    def test_empty_batch(self):
        ring = _ring(11, 4, 8).to(DEV)
        s, n = ops.framestack_gather(
            ring, t.empty(0, dtype=t.int64, device=DEV), 4
        )
        assert s.shape == n.shape == (0, 4, 4, 8)


class TestBufferOnDevice:
    def test_wrap_and_eviction_nchw(self):
        buf, batch = round_trip(DEV, stores=32)
        assert buf._planes.is_cuda and buf._inner.data["_base"].is_cuda
        for stack in (batch[0]["state"], batch[3]["state"]):
            assert stack.is_cuda and stack.is_contiguous()

    def test_wrap_and_eviction_nhwc(self):
        _, batch = round_trip(DEV, stores=12, frame_layout="nhwc")
        for stack in (batch[0]["state"], batch[3]["state"]):
            assert stack.is_cuda and stack.shape[1:] == (4, 4, 8)
            assert stack.is_contiguous(memory_format=t.channels_last)

    def test_prioritized_never_returns_dead(self):
        from util_framestack import (
            ATTRS, Episodes, RingModel, check_samples,
        )

        buf = DeviceFrameStackBuffer(40, DEV, prioritized=True)
        eps, model = Episodes(), RingModel(40)
        for length in [5, 7, 1, 9, 3, 12, 2, 6, 4]:
            episode, ids = eps.make(length)
            buf.store_episode(episode)
            model.store(ids)
        live = model.live()
        assert buf.size() == len(live)
        seen = set()
        for _ in range(10):
            _, batch, idx, w = buf.sample_batch(64, sample_attrs=ATTRS)
            assert idx.is_cuda and w.is_cuda
            seen |= check_samples(eps, batch, live)
        assert seen == live


def _pixelcatch_episodes(n, seed=0):
    from machin_amd.env.envs import PixelCatchEnv

    env = PixelCatchEnv(seed=seed, balls=1)
    rng = np.random.RandomState(seed)
    episodes = []
    for _ in range(n):
        obs, done, episode = env.reset(), False, []
        while not done:
            act = int(rng.randint(3))
            obs2, r, done, _ = env.step(act)
            episode.append({
                "state": {"state": t.from_numpy(obs).unsqueeze(0)},
                "action": {"action": t.tensor([[act]])},
                "next_state": {"state": t.from_numpy(obs2).unsqueeze(0)},
                "reward": r,
                "terminal": done,
            })
            obs = obs2
        episodes.append(episode)
    return episodes


@pytest.fixture(scope="module")
def episodes():
    return _pixelcatch_episodes(3)


class QNet(nn.Module):
    def __init__(self):
        super().__init__()
        from machin_amd.model.nets.nature_cnn import NatureCNN

        self.cnn = NatureCNN(4, feature_dim=128)
        self.head = nn.Linear(128, 3)

    def forward(self, state):
        return self.head(self.cnn(state.float() / 255.0))


class TestAlgorithmsOnFrameStackReplay:
    def test_dqn(self, episodes):
        from machin_amd.frame.algorithms import DQN

        dqn = DQN(
            QNet().to(DEV), QNet().to(DEV), t.optim.Adam, nn.MSELoss(),
            batch_size=32,
            replay_buffer=DeviceFrameStackBuffer(2000, DEV),
        )
        for episode in episodes:
            dqn.store_episode(episode)
        assert dqn.replay_buffer.size() == sum(map(len, episodes))
        losses = [dqn.update() for _ in range(5)]
        assert all(np.isfinite(v) for v in losses)

    def test_dqn_per(self, episodes):
        from machin_amd.frame.algorithms import DQNPer

        dqn = DQNPer(
            QNet().to(DEV), QNet().to(DEV), t.optim.Adam, nn.MSELoss(),
            batch_size=32,
            replay_buffer=DeviceFrameStackBuffer(
                2000, DEV, prioritized=True
            ),
        )
        for episode in episodes:
            dqn.store_episode(episode)
        losses = [dqn.update() for _ in range(5)]
        assert all(np.isfinite(v) for v in losses)
        assert dqn.replay_buffer._tree.weights.is_cuda


class TestNhwcFeedsFusedStem:
    def test_sampled_batch_runs_through_fused_cnn(self, episodes):
        from machin_amd.model.nets.nature_cnn import FusedActorCriticCNN

        bufs = {}
        for layout in ("nchw", "nhwc"):
            bufs[layout] = DeviceFrameStackBuffer(
                2000, DEV, frame_layout=layout
            )
            for episode in episodes:
                bufs[layout].store_episode(episode)
        # same generator state -> same sampled transitions
        stacks = {}
        for layout, buf in bufs.items():
            t.manual_seed(11)
            _, (state,) = buf.sample_batch(32, sample_attrs=["state"])
            stacks[layout] = state["state"]
        nhwc = stacks["nhwc"]
        assert nhwc.is_contiguous(memory_format=t.channels_last)
        converted = stacks["nchw"].contiguous(
            memory_format=t.channels_last
        )
        assert t.equal(nhwc, converted)
        assert nhwc.stride() == converted.stride()
        net = FusedActorCriticCNN(action_num=3).to(DEV)
        with t.no_grad():
            logits, value = net(nhwc)
            want_logits, want_value = net(converted)
        assert logits.shape == (32, 3)
        assert bool(t.isfinite(logits.float()).all())
        assert t.equal(logits, want_logits)
        assert t.equal(value, want_value)
