"""Frame-deduplicated replay on the CPU fallback path: semantics of
``ops.framestack_gather`` and the ``DeviceFrameStackBuffer`` ring
bookkeeping. Every comparison is exact (byte movement)."""
import numpy as np
import pytest
import torch as t

from machin_amd import ops
from machin_amd.frame.buffers import DeviceFrameStackBuffer
from util_framestack import (
    ATTRS, Episodes, RingModel, check_samples, round_trip,
)

P, H, W = 11, 4, 8
BASES = [0, 3, 6, 7, 10, 10]


def loop_reference(planes, base, k):
    """Literal per-sample definition of the op."""
    n_planes = planes.shape[0]
    state = t.empty((len(base), k, *planes.shape[1:]), dtype=t.uint8)
    next_state = t.empty_like(state)
    for b, s in enumerate(base):
        for j in range(k + 1):
            plane = planes[(s + j) % n_planes]
            if j < k:
                state[b, j] = plane
            if j >= 1:
                next_state[b, j - 1] = plane
    return state, next_state


@pytest.fixture(scope="module")
def ring():
    gen = t.Generator().manual_seed(1)
    return t.randint(0, 256, (P, H, W), dtype=t.uint8, generator=gen)


class TestFramestackGatherFallback:
    @pytest.mark.parametrize("channels_last", [False, True])
    @pytest.mark.parametrize("k", [1, 2, 4])
    @pytest.mark.parametrize(
        "bases", [BASES, [-1, -12, P, P + 2, 3 * P + 5, -(2 ** 40)]],
        ids=["wrap", "out_of_range"],
    )
    def test_matches_loop(self, ring, bases, k, channels_last):
        state, next_state = ops.framestack_gather(
            ring, t.tensor(bases), k, channels_last=channels_last
        )
        want_s, want_n = loop_reference(ring, bases, k)
        for got, want in ((state, want_s), (next_state, want_n)):
            assert got.dtype == t.uint8
            assert got.shape == (len(bases), k, H, W)
            assert t.equal(got, want)
            if channels_last:
                assert got.is_contiguous(memory_format=t.channels_last)
                if k > 1:
                    assert got.stride() == (H * W * k, 1, W * k, k)
            else:
                assert got.is_contiguous()

    def test_mod_rule(self, ring):
        """A negative base and a base >= P follow the mod-P rule."""
        s, n = ops.framestack_gather(ring, t.tensor([-1, P + 2]), 4)
        assert t.equal(s[0, 0], ring[P - 1]) and t.equal(s[0, 1], ring[0])
        assert t.equal(s[1, 0], ring[2]) and t.equal(n[1, 3], ring[6])

    def test_argument_checks(self, ring):
        with pytest.raises(ValueError):
            ops.framestack_gather(ring, t.tensor([0]), 0)
        with pytest.raises(ValueError):
            ops.framestack_gather(ring, t.tensor([0]), 9)
        with pytest.raises(ValueError):
            ops.framestack_gather(ring[:4], t.tensor([0]), 4)
        with pytest.raises(ValueError):
            ops.framestack_gather(ring.float(), t.tensor([0]), 4)


class TestFrameStackBufferRoundTrip:
    def test_wrap_and_eviction(self):
        buf, _ = round_trip("cpu", stores=32)
        # an episode that cannot fit the frame ring is refused
        episode, _ = Episodes().make(37)
        with pytest.raises(ValueError):
            buf.store_episode(episode)

    def test_nhwc_layout(self):
        _, batch = round_trip("cpu", stores=4, frame_layout="nhwc")
        for stack in (batch[0]["state"], batch[3]["state"]):
            assert stack.shape[1:] == (4, 4, 8)
            assert stack.is_contiguous(memory_format=t.channels_last)

    def test_store_transition_and_default_attrs(self):
        buf = DeviceFrameStackBuffer(40, "cpu")
        eps = Episodes()
        episode, _ = eps.make(3)
        for tr in episode:
            buf.store_transition(tr)  # 3 episodes of length 1
        assert buf.size() == 3
        n, batch = buf.sample_batch(16)
        # default order: sorted attrs + "*"
        action, next_state, reward, state, terminal, rest = batch
        assert rest == {} and reward.shape == (16, 1)
        check_samples(
            eps, (state, action, reward, next_state, terminal), {0, 1, 2}
        )


class TestFrameStackBufferValidation:
    def test_shuffled_episode(self):
        episode, _ = Episodes().make(6)
        shuffled = [episode[i] for i in (0, 1, 3, 2, 4, 5)]
        buf = DeviceFrameStackBuffer(40, "cpu")
        with pytest.raises(ValueError, match="step 1"):
            buf.store_episode(shuffled)
        assert buf.size() == 0
        loose = DeviceFrameStackBuffer(40, "cpu", validate=False)
        loose.store_episode(shuffled)
        assert loose.size() == 6

    def test_broken_window_inside_step(self):
        episode, _ = Episodes().make(4)
        episode[2]["next_state"]["state"] = (
            episode[2]["next_state"]["state"].flip(1)
        )
        with pytest.raises(ValueError, match="step 2"):
            DeviceFrameStackBuffer(40, "cpu").store_episode(episode)

    @pytest.mark.parametrize("bad", [
        t.zeros(1, 4, 4, 8),                      # not u8
        t.zeros(1, 3, 4, 8, dtype=t.uint8),       # wrong stack depth
        t.zeros(1, 4 * 4 * 8, dtype=t.uint8),     # not [1, k, H, W]
    ])
    def test_frame_tensor_shape(self, bad):
        episode, _ = Episodes().make(1)
        episode[0]["state"]["state"] = bad
        episode[0]["next_state"]["state"] = bad.clone()
        with pytest.raises(ValueError):
            DeviceFrameStackBuffer(40, "cpu").store_episode(episode)

    def test_changed_attributes_refused_without_side_effects(self):
        eps = Episodes()
        buf = DeviceFrameStackBuffer(40, "cpu")
        for length in (20, 10):
            buf.store_episode(eps.make(length)[0])
        episode, _ = eps.make(12)  # would evict if it were stored
        for tr in episode:
            tr["extra"] = 1.0
        with pytest.raises(ValueError, match="extra"):
            buf.store_episode(episode)
        assert buf.size() == 30
        _, batch = buf.sample_batch(500, sample_attrs=ATTRS)
        assert check_samples(eps, batch, set(range(30))) == set(range(30))

    def test_constructor_checks(self):
        with pytest.raises(ValueError):
            DeviceFrameStackBuffer(4, "cpu")  # needs k+1 frames
        with pytest.raises(ValueError):
            DeviceFrameStackBuffer(40, "cpu", frame_layout="hwc")
        with pytest.raises(ValueError):
            DeviceFrameStackBuffer(40, "cpu", frame_stack=9)


class TestEquivalenceWithStackedBuffer:
    def test_pixelcatch_stacks_identical(self):
        """Same seeded PixelCatch episodes in the stacked device buffer
        and in the frame ring: matching ids return identical stacks
        (zero padding at reset included)."""
        from machin_amd.env.envs import PixelCatchEnv
        from machin_amd.frame.buffers import DeviceTransitionBuffer

        stacked = DeviceTransitionBuffer(512, "cpu")
        dedup = DeviceFrameStackBuffer(512, "cpu")
        env = PixelCatchEnv(seed=3, balls=1)
        rng = np.random.RandomState(3)
        tid = 0
        for _ in range(2):
            obs, done, episode = env.reset(), False, []
            while not done:
                act = int(rng.randint(3))
                obs2, _, done, _ = env.step(act)
                episode.append({
                    "state": {"state": t.from_numpy(obs).unsqueeze(0)},
                    "action": {"action": t.tensor([[act]])},
                    "next_state": {
                        "state": t.from_numpy(obs2).unsqueeze(0)
                    },
                    "reward": float(tid),
                    "terminal": done,
                })
                tid += 1
                obs = obs2
            stacked.store_episode(episode)
            dedup.store_episode(episode)
        assert dedup.size() == stacked.size() == tid

        def by_id(buf):
            _, (state, reward, next_state) = buf.sample_batch(
                400, sample_attrs=["state", "reward", "next_state"]
            )
            out = {}
            for i, r in enumerate(reward.view(-1).long().tolist()):
                out[r] = (state["state"][i], next_state["state"][i])
            return out

        a, b = by_id(stacked), by_id(dedup)
        common = set(a) & set(b)
        assert len(common) > tid // 2
        for i in common:
            assert t.equal(a[i][0], b[i][0]) and t.equal(a[i][1], b[i][1])


class TestPrioritizedFrameStackBuffer:
    def _filled(self, stores=9):
        buf = DeviceFrameStackBuffer(40, "cpu", prioritized=True)
        eps, model = Episodes(), RingModel(40)
        for length in [5, 7, 1, 9, 3, 12, 2, 6, 4][:stores]:
            episode, ids = eps.make(length)
            buf.store_episode(episode)
            model.store(ids)
        return buf, eps, model

    def test_dead_ids_never_sampled(self):
        buf, eps, model = self._filled()
        live = model.live()
        assert buf.size() == len(live) < len(eps.state)  # evicted some
        seen = set()
        for _ in range(50):
            n, batch, idx, is_weight = buf.sample_batch(
                64, sample_attrs=ATTRS
            )
            assert n == 64 and idx.shape == (64,)
            assert is_weight.shape == (64,)
            assert bool(t.isfinite(is_weight).all())
            assert float(is_weight.max()) == 1.0
            seen |= check_samples(eps, batch, live)
        assert seen == live

    def test_priority_update_skews_sampling(self):
        buf, eps, _ = self._filled(stores=2)  # 12 live, nothing evicted
        target = 8
        _, (reward,), idx, _ = buf.sample_batch(
            256, sample_attrs=["reward"]
        )
        slot = idx[reward.view(-1) == target][0]
        buf.update_priority(t.tensor([1000.0]), slot.view(1))
        _, (reward,), idx, _ = buf.sample_batch(
            64, sample_attrs=["reward"]
        )
        assert int((reward.view(-1) == target).sum()) > 32

    def test_update_of_evicted_slot_stays_dead(self):
        buf, eps, model = self._filled()
        tail = (buf._t_count - buf._live) % buf._t_capacity
        dead_slot = (tail - 1) % buf._t_capacity
        buf.update_priority(t.tensor([1000.0]), t.tensor([dead_slot]))
        live = model.live()
        for _ in range(10):
            _, batch, _, _ = buf.sample_batch(64, sample_attrs=ATTRS)
            check_samples(eps, batch, live)

    def test_clear(self):
        buf, eps, model = self._filled()
        buf.clear()
        assert buf.size() == 0 and len(buf) == 0
        assert buf.sample_batch(8) == (0, None, None, None)
        episode, ids = eps.make(5)
        buf.store_episode(episode)
        assert buf.size() == 5
        _, batch, _, _ = buf.sample_batch(64, sample_attrs=ATTRS)
        assert check_samples(eps, batch, set(ids)) == set(ids)

    def test_uniform_clear(self):
        buf, _ = round_trip("cpu", stores=3)
        buf.clear()
        assert buf.size() == 0 and buf.sample_batch(8) == (0, None)
