"""CPU tests of the device-resident PixelCatch: the torch fallback of
``ops.pixelcatch_step`` behind ``DevicePixelCatchVecEnv(device="cpu")``
against the host ``PixelCatchEnv`` driven by an independent Philox
(util_pixelcatch_device), the episode recorder against the oracle's
episodes, and ``DeviceFrameStackBuffer.store_frames`` against
``store_episode``. Every comparison is ``torch.equal``."""
import pytest
import torch as t

from machin_amd import ops
from machin_amd.env.envs import DevicePixelCatchVecEnv, PixelCatchEnv
from machin_amd.env.wrappers.base import ParallelWrapperBase
from machin_amd.frame.buffers import DeviceFrameStackBuffer
from util_pixelcatch_device import (
    PHILOX_KNOWN_ANSWERS, SEED, assert_same_batches, check_finished,
    oracle_trace, philox4x32_10, replay_trace, spawn_x,
)

LAYOUTS = ["nchw", "nhwc"]


def make_env(num_envs, device="cpu", **kwargs):
    kwargs.setdefault("seed", SEED)
    kwargs.setdefault("balls", 2)
    return DevicePixelCatchVecEnv(num_envs, device, **kwargs)


class TestPhilox:
    def test_oracle_known_answers(self):
        for counter, key, want in PHILOX_KNOWN_ANSWERS:
            assert philox4x32_10(counter, key) == want

    def test_fallback_matches_oracle(self):
        zero = t.zeros(1, dtype=t.int64)
        assert ops._philox4x32_10_first(0, zero, zero).tolist() == [
            PHILOX_KNOWN_ANSWERS[0][2][0]
        ]
        # the tensor version takes 64-bit (offset, subsequence) pairs
        # that fit int64: compare with the python one on such counters
        seeds = [0, SEED, 2 ** 64 - 1]
        offs = [0, 1, 77, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 12345,
                2 ** 62 + 3]
        subs = [0, 1, 64, 2048, 2 ** 31, 2 ** 33 + 5]
        for seed in seeds:
            off = t.tensor([o for o in offs for _ in subs])
            sub = t.tensor([s for _ in offs for s in subs])
            got = ops._philox4x32_10_first(seed, off, sub).tolist()
            want = [
                philox4x32_10((o & 0xFFFFFFFF, o >> 32, s & 0xFFFFFFFF,
                               s >> 32), (seed & 0xFFFFFFFF, seed >> 32))[0]
                for o in offs for s in subs
            ]
            assert got == want

    def test_spawn_range(self):
        xs = [spawn_x(SEED, e, n) for e in range(8) for n in range(200)]
        assert min(xs) == 3 and max(xs) == 80


class TestFallbackAgainstOracle:
    @pytest.mark.parametrize("layout", LAYOUTS)
    @pytest.mark.parametrize("num_envs", [1, 3, 16])
    def test_two_auto_resets(self, num_envs, layout):
        # balls=2: every episode is 54 steps, so 120 steps cross two
        # auto-resets
        trace = oracle_trace(num_envs, 120)
        assert sum(len(e) for e in trace.episodes) == 2 * num_envs
        assert all(len(ep) == 54 for e in trace.episodes for _, ep in e)
        rewards = t.stack(trace.reward)
        print("rewards +1:", int((rewards == 1).sum()),
              "-1:", int((rewards == -1).sum()))
        assert bool((rewards == 1).any())  # even envs track the ball
        if num_envs >= 3:  # odd envs act at random and mostly miss
            assert bool((rewards == -1).any())
        replay_trace(make_env(num_envs, layout=layout), trace)

    @pytest.mark.parametrize("layout", LAYOUTS)
    def test_max_episode_steps(self, layout):
        trace = oracle_trace(3, 50, balls=5, max_episode_steps=20)
        assert [len(e) for e in trace.episodes].count(3) == 2
        replay_trace(
            make_env(3, balls=5, max_episode_steps=20, layout=layout), trace
        )

    def test_ball_lands_on_the_step_limit(self):
        # step 27 lands a ball AND hits the limit: spawn, then reset
        trace = oracle_trace(3, 60, balls=5, max_episode_steps=27)
        replay_trace(make_env(3, balls=5, max_episode_steps=27), trace)

    @pytest.mark.parametrize("layout", LAYOUTS)
    def test_no_auto_reset_with_partial_reset(self, layout):
        kwargs = dict(balls=1, auto_reset=False,
                      resets=((30, (0, 2)), (40, (1,)), (45, (1, 3))))
        trace = oracle_trace(4, 70, **kwargs)
        # latched steps are in the trace
        assert float(t.stack(trace.done).sum()) > 8
        env = make_env(4, balls=1, auto_reset=False, layout=layout)

        def check_active(step):
            want = [e for e in range(4) if trace.done[step][e] == 0]
            assert env.active() == want

        replay_trace(env, trace, check_active)

    def test_reset_with_index_tensor(self):
        env_a, env_b = make_env(5), make_env(5)
        env_a.reset()
        env_b.reset()
        obs_a = env_a.reset([1, 3]).clone()
        obs_b = env_b.reset(t.tensor([3, 1, 3, 99, -1]))
        assert t.equal(obs_a, obs_b)
        assert t.equal(env_a.ball_no, env_b.ball_no)
        assert env_a.ball_no.tolist() == [1, 2, 1, 2, 1]

    def test_out_of_range_actions_are_clamped(self):
        trace = oracle_trace(4, 60, wild_actions=True)
        acts = t.stack(trace.actions)
        assert int(acts.min()) < 0 and int(acts.max()) > 2
        replay_trace(make_env(4), trace)

    def test_seed_reproduces(self):
        trace = oracle_trace(3, 40)
        env = make_env(3, seed=7)
        env.reset()
        for action in trace.actions[:30]:
            env.step(action)
        assert env.seed(SEED) == [SEED]
        assert env.ball_no.tolist() == [0, 0, 0]
        replay_trace(env, trace)
        other = oracle_trace(3, 40, seed=7)
        assert not t.equal(other.first_obs, trace.first_obs)

    @pytest.mark.parametrize("layout", LAYOUTS)
    def test_paddle_at_both_walls(self, layout):
        replay_trace(make_env(2, layout=layout),
                     oracle_trace(2, 30, policy="edges"))

    def test_edges_were_rendered(self):
        # ball_y = 0 (clipped top row), ball_y = 81 (ball in the paddle
        # rows), paddle at 4 and at 80 all occur in the compared traces
        frames = t.stack(oracle_trace(16, 120).frame)  # [T, E, 84, 84]
        assert bool((frames[:, :, 0] == 255).any())
        # a landed ball away from the paddle: two runs in row 81
        row = frames[:, :, 81]
        assert bool(((row[..., 1:] != row[..., :-1]).sum(-1) >= 3).any())
        frames = t.stack(oracle_trace(2, 30, policy="edges").frame)
        assert bool((frames[:, :, 81:, 0] == 255).any())   # paddle at 4
        assert bool((frames[:, :, 81:, 83] == 255).any())  # paddle at 80


class TestInterface:
    def test_spaces_and_base_class(self):
        env = make_env(2)
        host = PixelCatchEnv()
        assert isinstance(env, ParallelWrapperBase)
        assert env.size() == 2
        assert env.observation_space.shape == host.observation_space.shape
        assert env.action_space.n == host.action_space.n
        assert env.paddle_x.dtype == t.int32 and env.ball_no.dtype == t.int64
        env.reset()
        assert env.active() == [0, 1]
        assert t.equal(env.render(), env.reset()[:, -1])
        env.close()
        with pytest.raises(RuntimeError):
            env.reset()

    def test_argument_errors(self):
        for bad in (dict(num_envs=0), dict(layout="hwc"), dict(balls=0),
                    dict(max_episode_steps=0)):
            kwargs = {"num_envs": 2, "device": "cpu", **bad}
            with pytest.raises(ValueError):
                DevicePixelCatchVecEnv(**kwargs)
        env = make_env(3)
        with pytest.raises(RuntimeError, match="reset"):
            env.step(t.zeros(3, dtype=t.int64))
        env.reset()
        env.step(t.zeros(3, dtype=t.int64))
        env.step(t.zeros((3, 1), dtype=t.int32))
        for bad in (
            t.zeros(3), t.zeros(3, dtype=t.bool), t.zeros(4, dtype=t.int64),
            t.zeros((1, 3), dtype=t.int64), [0, 1, 2],
            t.zeros(3, dtype=t.int64, device="meta"),
        ):
            with pytest.raises(ValueError):
                env.step(bad)
        with pytest.raises(ValueError):
            env.reset([3])
        with pytest.raises(ValueError):
            env.reset(t.tensor([0], dtype=t.int32))
        with pytest.raises(RuntimeError, match="record"):
            env.finished_episodes()

    def test_op_argument_errors(self):
        env = make_env(2, record=True)
        env.reset()
        good = dict(
            state=env._state, ball_no=env._ball_no,
            action=t.zeros(2, dtype=t.int64), obs=env._obs,
            frame=env._frame, reward=env._reward, done=env._done,
            ep_len=env._ep_len, seed=1, balls=2, max_episode_steps=10,
            auto_reset=True, log=env._log,
        )
        ops.pixelcatch_step(**good)
        for bad in (
            dict(state=env._state.long()), dict(state=env._state[:, :9]),
            dict(ball_no=env._ball_no.int()),
            dict(action=t.zeros(3, dtype=t.int64)),
            dict(action=t.zeros(2, dtype=t.int32)),
            dict(obs=env._obs[:, :3]), dict(obs=env._obs.float()),
            dict(obs=env._obs.transpose(2, 3)),
            dict(frame=env._frame[:1]), dict(reward=env._reward.double()),
            dict(done=env._done[:1]), dict(ep_len=env._ep_len.long()),
            dict(balls=0), dict(max_episode_steps=0),
            dict(log=env._log[:3]),
            dict(log=(env._log[0][:, :4],) + env._log[1:]),
            dict(log=(env._log[0], env._log[1][:, :5]) + env._log[2:]),
        ):
            with pytest.raises(ValueError):
                ops.pixelcatch_step(**{**good, **bad})
        with pytest.raises(ValueError):
            ops.pixelcatch_reset(env._state, env._ball_no,
                                 t.ones(3, dtype=t.uint8), env._obs, 1, 2)


class TestRecorder:
    def test_views_equal_oracle_episodes(self):
        trace = oracle_trace(3, 120)
        env = make_env(3, record=True)
        assert env.max_len == 54
        seen = []

        def on_step(step):
            got = env.finished_episodes()
            seen.extend(check_finished(got, trace.episodes[step]))
            for frames, _ in got:  # views of the log, not copies
                assert frames.data_ptr() >= env._log[0].data_ptr()
                assert frames._base is not None

        replay_trace(env, trace, on_step)
        assert len(seen) == 6

    def test_step_limit_and_no_auto_reset(self):
        trace = oracle_trace(3, 50, balls=5, max_episode_steps=20)
        env = make_env(3, balls=5, max_episode_steps=20, record=True)
        assert env.max_len == 20
        replay_trace(env, trace, lambda step: check_finished(
            env.finished_episodes(), trace.episodes[step]))
        kwargs = dict(balls=1, auto_reset=False, resets=((30, (0, 2)),))
        trace = oracle_trace(3, 60, **kwargs)
        env = make_env(3, balls=1, auto_reset=False, record=True)
        # a latched env is reported once, in the step that ended it
        replay_trace(env, trace, lambda step: check_finished(
            env.finished_episodes(), trace.episodes[step]))


class TestStoreFrames:
    @pytest.mark.parametrize("prioritized", [False, True],
                             ids=["uniform", "per"])
    @pytest.mark.parametrize("n_step", [1, 3])
    def test_equals_store_episode_with_wrap(self, n_step, prioritized):
        # 100 frame slots, episodes of 54 + 4: the second store wraps
        # the ring and evicts part of the first
        trace = oracle_trace(3, 120)
        env = make_env(3, record=True)
        kwargs = dict(n_step=n_step, prioritized=prioritized, discount=0.5)
        by_frames = DeviceFrameStackBuffer(100, "cpu", **kwargs)
        by_episode = DeviceFrameStackBuffer(100, "cpu", **kwargs)
        stores = []

        def on_step(step):
            for frames, cols in check_finished(env.finished_episodes(),
                                               trace.episodes[step]):
                by_frames.store_frames(frames, cols)
            for _, episode in trace.episodes[step]:
                by_episode.store_episode(episode)
            if trace.episodes[step]:
                stores.append(by_frames.size())
                assert_same_batches(by_frames, by_episode)

        replay_trace(env, trace, on_step)
        assert len(stores) == 2 and stores[-1] < 6 * 54
        assert by_frames._plane_count == by_episode._plane_count == 6 * 58
        assert list(by_frames._episodes) == list(by_episode._episodes)
        if prioritized:
            assert t.equal(by_frames._tree.weights,
                           by_episode._tree.weights)

    def test_custom_column_and_errors(self):
        buf = DeviceFrameStackBuffer(40, "cpu")
        frames = t.randint(0, 256, (9, 6, 8), dtype=t.uint8)
        cols = {
            "action/action": t.zeros((5, 1), dtype=t.int64),
            "reward": t.arange(5, dtype=t.float32),
            "terminal": t.zeros(5),
            "tid": t.arange(5, dtype=t.float32),
        }
        buf.store_frames(frames, cols)
        assert buf.size() == 5
        _, (state, _, reward, next_state, _, others) = buf.sample_batch(
            32, sample_attrs=["state", "action", "reward", "next_state",
                              "terminal", "*"])
        ids = others["tid"].long().view(-1)
        assert t.equal(reward.view(-1), cols["reward"][ids])
        for b, i in enumerate(ids.tolist()):
            assert t.equal(state["state"][b], frames[i : i + 4])
            assert t.equal(next_state["state"][b], frames[i + 1 : i + 5])
        for bad_frames, bad_cols in (
            (frames.float(), cols), (frames[:4], cols), (frames[0], cols),
            (frames, {**cols, "reward": cols["reward"][:4]}),
            (frames, {**cols, "state/state": frames[:5]}),
            (frames, {**cols, "_base": t.arange(5)}),
            (frames, {k: v for k, v in cols.items() if k != "tid"}),
            (frames[:, :5], cols),
            (t.zeros((60, 6, 8), dtype=t.uint8), cols),
        ):
            with pytest.raises(ValueError):
                buf.store_frames(bad_frames, bad_cols)
        assert buf.size() == 5
