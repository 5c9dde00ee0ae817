"""GPU tests for the random-shift (DrQ) augmentation fused into the
frame-stack gather: the gfx950 shifted kernels (1-step and n-step)
against the torch fallback, byte for byte and stride for stride, the
binding's argument checks, ``DeviceFrameStackBuffer(augment_shift=...)``
on ``cuda:0`` and RAINBOW training from it."""
import numpy as np
import pytest
import torch as t
import torch.nn as nn

pytestmark = pytest.mark.gpu

if not t.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from machin_amd import ops  # noqa: E402
from machin_amd.frame.buffers import DeviceFrameStackBuffer  # noqa: E402
from util_framestack_shift import (  # noqa: E402
    check_buffer, check_strides, kernel_shift_rows, random_shift, ring,
)

DEV = "cuda:0"
LAYOUTS = pytest.mark.parametrize("channels_last", [False, True],
                                  ids=["nchw", "nhwc"])


def _check(planes, base, k, channels_last, shift, planes_dev=None):
    """Kernel output == CPU fallback output, byte for byte."""
    base = t.as_tensor(base, dtype=t.int64)
    want = ops.framestack_gather(planes, base, k, channels_last,
                                 shift=shift)
    planes_dev = planes.to(DEV) if planes_dev is None else planes_dev
    got = ops.framestack_gather(planes_dev, base.to(DEV), k, channels_last,
                                shift=shift.to(DEV))
    for g, w in zip(got, want):
        assert g.is_cuda
        check_strides(g, w, channels_last)
        assert t.equal(g.cpu(), w)
    return got


@LAYOUTS
class TestKernelMatchesFallback:
    def test_vector_path(self, channels_last):
        base, shift = kernel_shift_rows()
        _check(ring(11, 4, 8), base, 4, channels_last, shift)

    def test_width_12_interior_dwords_on_both_sides(self, channels_last):
        base, shift = kernel_shift_rows()
        _check(ring(11, 4, 12), base, 4, channels_last, shift)

    def test_scalar_path(self, channels_last):
        base, shift = kernel_shift_rows()
        _check(ring(11, 3, 5), base, 4, channels_last, shift)

    def test_unaligned_ring_takes_scalar_path(self, channels_last):
        planes = ring(11, 4, 8)
        flat = t.empty(11 * 32 + 1, dtype=t.uint8, device=DEV)
        view = flat[1:].view(11, 4, 8)
        view.copy_(planes)
        assert view.data_ptr() % 4 != 0
        base, shift = kernel_shift_rows()
        _check(planes, base, 4, channels_last, shift, planes_dev=view)

    @pytest.mark.parametrize("k", [1, 2, 8])
    def test_other_stack_depths(self, channels_last, k):
        # NHWC with k != 4 is the generic interleave
        base, shift = kernel_shift_rows()
        _check(ring(11, 4, 8), base, k, channels_last, shift)

    def test_atari_small_batch(self, channels_last):
        _check(ring(64, 84, 84), [0, 61, 63], 4, channels_last,
               random_shift(3, 4, seed=1))

    def test_atari_grid_stride(self, channels_last):
        # 1200 * 1764 work items > 2048 blocks * 256 threads
        gen = t.Generator().manual_seed(5)
        base = t.randint(0, 64, (1200,), generator=gen)
        _check(ring(64, 84, 84), base, 4, channels_last,
               random_shift(1200, 4, seed=2))

    def test_zero_and_none_are_the_unshifted_kernel(self, channels_last):
        planes, (base, shift) = ring(11, 4, 8).to(DEV), kernel_shift_rows()
        base = base.to(DEV)
        want = ops.framestack_gather(planes, base, 4, channels_last)
        for s in (None, t.zeros_like(shift).to(DEV)):
            got = ops.framestack_gather(planes, base, 4, channels_last,
                                        shift=s)
            for g, w in zip(got, want):
                assert t.equal(g, w) and g.stride() == w.stride()

    def test_side_stream(self, channels_last):
        planes = ring(64, 84, 84)
        base, shift = t.tensor([5, 62, 0, 33]), random_shift(4, 4, seed=3)
        want = ops.framestack_gather(planes, base, 4, channels_last,
                                     shift=shift)
        planes_dev, base_dev = planes.to(DEV), base.to(DEV)
        shift_dev = shift.to(DEV)
        side = t.cuda.Stream()
        side.wait_stream(t.cuda.current_stream())
        with t.cuda.stream(side):
            got = ops.framestack_gather(planes_dev, base_dev, 4,
                                        channels_last, shift=shift_dev)
        side.synchronize()
        assert t.equal(got[0].cpu(), want[0])
        assert t.equal(got[1].cpu(), want[1])


def _nstep_case():
    """Ring (11, 4, 8), 12 transitions in episodes of 5, 4 and 3 steps:
    with n = 3, ``left`` gives windows of m = 1, 2 and 3. Integer
    rewards and gamma 0.5 keep every fp32 partial sum exact."""
    gen = t.Generator().manual_seed(9)
    base, shift = kernel_shift_rows()
    return dict(
        planes=ring(11, 4, 8),
        base=t.randint(0, 11, (12,), generator=gen),
        left=t.tensor([4, 3, 2, 1, 0, 3, 2, 1, 0, 2, 1, 0]),
        reward=t.randint(-3, 4, (12,), generator=gen).float(),
        terminal=t.tensor([0, 0, 0, 0, 1, 0, 1, 0, 1, 0, 0, 1.0]),
        pos=t.arange(len(base)) % 12,
        shift=shift,
    )


def _nstep(case, k, channels_last, device, shift="case"):
    cols = [case[name].to(device) for name in
            ("planes", "base", "left", "reward", "terminal", "pos")]
    if isinstance(shift, str):
        shift = case["shift"].to(device)
    return ops.framestack_gather_nstep(
        *cols, k, 3, 0.5, channels_last=channels_last, shift=shift
    )


@LAYOUTS
class TestNStepKernelMatchesFallback:
    @pytest.mark.parametrize("k", [2, 4])
    def test_stacks_and_scalars(self, channels_last, k):
        case = _nstep_case()
        want = _nstep(case, k, channels_last, "cpu")
        got = _nstep(case, k, channels_last, DEV)
        assert set(want[4].tolist()) == {1, 2, 3}
        for g, w in zip(got[:2], want[:2]):
            assert g.is_cuda
            check_strides(g, w, channels_last)
            assert t.equal(g.cpu(), w)
        plain = _nstep(case, k, channels_last, DEV, shift=None)
        for i in (2, 3, 4):
            assert got[i].dtype == want[i].dtype
            assert t.equal(got[i].cpu(), want[i])
            assert t.equal(got[i], plain[i])

    def test_scalar_path(self, channels_last):
        case = dict(_nstep_case(), planes=ring(11, 3, 5))
        want = _nstep(case, 4, channels_last, "cpu")
        got = _nstep(case, 4, channels_last, DEV)
        for g, w in zip(got, want):
            assert t.equal(g.cpu(), w)

    def test_zero_and_none_are_the_unshifted_kernel(self, channels_last):
        case = _nstep_case()
        want = _nstep(case, 4, channels_last, DEV, shift=None)
        zero = t.zeros_like(case["shift"]).to(DEV)
        got = _nstep(case, 4, channels_last, DEV, shift=zero)
        assert all(t.equal(g, w) for g, w in zip(got, want))
        assert got[0].stride() == want[0].stride()


class TestBindingChecks:
    def test_rejects_bad_shift(self):
        planes = ring(11, 4, 8).to(DEV)
        base = t.tensor([0, 3, 6], device=DEV)
        good = t.zeros((3, 4), dtype=t.int32, device=DEV)
        case = _nstep_case()
        case["pos"], case["shift"] = case["pos"][:3], good
        ops.framestack_gather(planes, base, 4, shift=good)
        _nstep(case, 4, False, DEV)
        wide = t.zeros((3, 8), dtype=t.int32, device=DEV)
        for bad in (
            good.long(),  # int64
            good[:, :2].contiguous(),  # [B, 2]
            wide[:, ::2],  # [B, 4], not contiguous
            good.cpu(),  # another device
            good[:2],  # wrong B
        ):
            with pytest.raises(RuntimeError):
                ops.framestack_gather(planes, base, 4, shift=bad)
            with pytest.raises(RuntimeError):
                _nstep(case, 4, False, DEV, shift=bad)

    def test_positional_calls_are_unchanged(self):
        ext = ops._require_ext()
        planes = ring(11, 4, 8).to(DEV)
        base = t.tensor([0, 3, 6], device=DEV)
        s, n = ext.framestack_gather(planes, base, 4, False)
        assert s.shape == n.shape == (3, 4, 4, 8)

    def test_empty_batch(self):
        planes = ring(11, 4, 8).to(DEV)
        empty = t.empty((0, 4), dtype=t.int32, device=DEV)
        s, n = ops.framestack_gather(
            planes, t.empty(0, dtype=t.int64, device=DEV), 4, shift=empty
        )
        assert s.shape == n.shape == (0, 4, 4, 8)
        case = _nstep_case()
        case["pos"] = case["pos"][:0]
        out = _nstep(case, 4, True, DEV, shift=empty)
        assert out[0].shape == out[1].shape == (0, 4, 4, 8)
        assert out[2].shape == out[3].shape == out[4].shape == (0,)


class TestBufferOnDevice:
    @pytest.mark.parametrize("layout", ["nchw", "nhwc"])
    @pytest.mark.parametrize("prioritized", [False, True],
                             ids=["uniform", "per"])
    @pytest.mark.parametrize("n_step", [1, 3])
    def test_on_shifts_the_original_stacks(self, n_step, prioritized,
                                           layout):
        buf, shift = check_buffer(DEV, n_step, prioritized, layout)
        assert buf._planes.is_cuda
        assert shift.is_cuda and shift.dtype == t.int32

    def test_off_returns_no_shift(self):
        from util_framestack import ATTRS, Episodes

        buf = DeviceFrameStackBuffer(40, DEV, augment_shift=0)
        buf.store_episode(Episodes().make(5)[0])
        _, batch = buf.sample_batch(8, sample_attrs=ATTRS + ["*"])
        assert batch[5] == {}


class PixelDistQNet(nn.Module):
    """Tiny conv C51 net on [B, 4, 84, 84] u8 stacks; probabilities."""

    def __init__(self, action_num=3, atom_num=11):
        super().__init__()
        self.action_num, self.atom_num = action_num, atom_num
        self.conv = nn.Conv2d(4, 4, 12, stride=12)
        self.fc = nn.Linear(4 * 7 * 7, action_num * atom_num)

    def forward(self, state):
        a = t.relu(self.conv(state.float() / 255.0)).flatten(1)
        a = self.fc(a).view(-1, self.action_num, self.atom_num)
        return t.softmax(a, dim=-1)


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
                "reward": float(r),
                "terminal": done,
            })
            obs = obs2
        episodes.append(episode)
    return episodes


class TestRainbowOnDevice:
    def test_three_updates_with_augmentation(self):
        from machin_amd.frame.algorithms import RAINBOW

        buf = DeviceFrameStackBuffer(
            2000, "cuda:0", prioritized=True, n_step=3, discount=0.99,
            augment_shift=4,
        )
        algo = RAINBOW(
            PixelDistQNet().to(DEV), PixelDistQNet().to(DEV), t.optim.Adam,
            -5.0, 5.0, batch_size=32, reward_future_steps=3, discount=0.99,
            replay_buffer=buf, fused_loss=True, dist_from_logits=False,
        )
        episodes = _pixelcatch_episodes(3)
        for episode in episodes:
            algo.store_episode(episode)
        assert buf.size() == sum(map(len, episodes))
        losses = [algo.update() for _ in range(3)]
        assert all(np.isfinite(v) for v in losses)
        _, batch, _, _ = buf.sample_batch(32, sample_attrs=["state", "*"])
        assert batch[0]["state"].shape == (32, 4, 84, 84)
        assert {"n_step", "shift"} <= set(batch[1])
        assert batch[1]["shift"].is_cuda
