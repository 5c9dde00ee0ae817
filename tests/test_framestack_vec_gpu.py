"""GPU tests of the per-step vector-env store: the gfx950
``framestack_vec_append`` kernel against its torch fallback after every
step of scripted runs and against the ledger of util_framestack_vec at
the end, its byte and channels_last paths against the vector path, the
same env steps stored through the existing episode path, and RAINBOW
learning from the buffer. Every comparison is ``torch.equal``."""
import pytest
import torch as t
import torch.nn as nn

pytestmark = pytest.mark.gpu

if not t.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from machin_amd import ops  # noqa: E402
from machin_amd.env.envs import DevicePixelCatchVecEnv  # noqa: E402
from machin_amd.frame.algorithms import RAINBOW  # noqa: E402
from machin_amd.frame.buffers import DeviceVecFrameStackBuffer  # noqa: E402
from util_framestack_vec import (  # noqa: E402
    ENDS, FRAMES, Ledger, append_op, check_ledger, env_against_episode_path,
    feed, feed_ledger, make_buffer, ring_state, stream,
)

DEV = "cuda:0"
NAMES = ["planes", "reward", "terminal", "left", "head", "run", "action",
         "tree", "pos", "leaf_idx", "leaf_w"]


def same(a, b):
    """torch.equal as a device flag (no wait for the device)."""
    assert a.shape == b.shape and a.dtype == b.dtype
    return (a == b).all()


def kernel_against_fallback(E, H, W, k, n, S, steps, kind, **feed_kwargs):
    """Drive one buffer through the kernel and one through the torch
    fallback with the same stream; compare everything after every step
    and the kernel's buffer with the ledger at the end."""
    hip, ref = make_buffer(E, S, k, n, DEV), make_buffer(E, S, k, n, DEV)
    ledger = Ledger(E, S, k, n)
    flags = []
    for item in stream(E, H, W, k, S, steps, kind, k + n):
        out_hip, out_ref = [], []
        with append_op(ops.framestack_vec_append, out_hip):
            feed(hip, item, **feed_kwargs)
        with append_op(ops._framestack_vec_append_torch, out_ref):
            feed(ref, item)
        feed_ledger(ledger, item)
        if item[0] != "step":
            continue
        a = list(ring_state(hip).values()) + list(out_hip[0])
        b = list(ring_state(ref).values()) + list(out_ref[0])
        flags.append(t.stack([same(x, y) for x, y in zip(a, b)]))
    flags = t.stack(flags).cpu()
    bad = (~flags).nonzero()
    assert bad.numel() == 0, (
        f"step {int(bad[0, 0])}: {NAMES[int(bad[0, 1])]} differs from the "
        f"fallback"
    )
    assert check_ledger(hip, ledger) > 0
    return hip, ref


class TestKernelAgainstFallback:
    @pytest.mark.parametrize("kind", ENDS)
    @pytest.mark.parametrize("extra", [0, 5])
    @pytest.mark.parametrize("n", [1, 3])
    @pytest.mark.parametrize("k", [1, 4])
    @pytest.mark.parametrize("frame", FRAMES)
    def test_scripted_run(self, frame, k, n, extra, kind):
        S = 2 * (k + n) + extra
        kernel_against_fallback(3, *frame, k, n, S, 6 * S + 7, kind)

    def test_more_than_one_wave_of_lanes(self):
        # 84 x 84: the 16-byte path, 441 chunks per plane
        kernel_against_fallback(65, 84, 84, 4, 3, 20, 50, "p15")

    def test_byte_path_of_an_unaligned_frame(self):
        """A frame that starts 4 bytes into a larger tensor takes the
        byte path; the ring is the one of the aligned frame (which the
        fallback was compared with above)."""
        def view(frame):
            big = t.empty(frame.numel() + 16, dtype=t.uint8, device=DEV)
            off = big[4:4 + frame.numel()].view(frame.shape)
            assert off.data_ptr() % 16 == 4
            return off.copy_(frame)

        kernel_against_fallback(65, 84, 84, 4, 3, 20, 30, "p15",
                                frame_view=view)

    @pytest.mark.parametrize("frame", [(84, 84), (5, 7)])
    def test_first_channels_last(self, frame):
        kernel_against_fallback(5, *frame, 4, 3, 19, 60, "p60",
                                channels_last=True)


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
def test_against_the_episode_path(layout):
    got, want, vec = env_against_episode_path(DEV, layout)
    assert len(want) == 162 and len(got) == 162
    assert got == want
    assert vec.size() == 162


class SmallDistQNet(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(4, 8, 8, stride=8)
        self.head = nn.Linear(8 * 10 * 10, 3 * 11)

    def forward(self, state):
        x = t.relu(self.conv(state.float() / 255.0)).flatten(1)
        return t.softmax(self.head(x).view(-1, 3, 11), dim=-1)


def test_rainbow_learns_from_the_buffer():
    t.manual_seed(0)
    buffer = DeviceVecFrameStackBuffer(
        8, 64, DEV, prioritized=True, n_step=3, discount=0.99,
        augment_shift=4,
    )
    rainbow = RAINBOW(
        SmallDistQNet().to(DEV), SmallDistQNet().to(DEV), t.optim.Adam,
        -2.0, 2.0, batch_size=16, reward_future_steps=3, discount=0.99,
        replay_buffer=buffer,
    )
    env = DevicePixelCatchVecEnv(8, DEV, balls=1)
    obs = env.reset()
    buffer.begin(obs)
    leaves = buffer._tree.get_leaf_all_weights()
    losses, changed = [], []
    for step in range(40):
        action = t.randint(0, 3, (8,), device=DEV)
        obs, reward, done, info = env.step(action)
        buffer.append_step(action, reward, done, info["frame"], obs)
        if step >= 10:
            before = leaves.clone()
            losses.append(rainbow.update())
            changed.append((leaves != before).any())
    assert all(loss == loss and abs(loss) < float("inf") for loss in losses)
    assert len(losses) == 30 and all(bool(c) for c in changed)
    assert buffer.size() == int((leaves > 0).sum()) > 0
    assert buffer.steps_stored == 40
