"""Device-resident batched PixelCatch.

No reference counterpart. :class:`.pixel_catch.PixelCatchEnv` renders
with numpy on the host, one env per object; a learner that samples
millions of transitions per second from HBM replay is then bound by the
env and by per-transition python. PixelCatch is an integer function of
three small numbers per frame (paddle x, ball x, ball y), so
:class:`DevicePixelCatchVecEnv` keeps the state of thousands of envs in
HBM and steps and renders all of them with one gfx950 kernel
(:func:`machin_amd.ops.pixelcatch_step`) that writes the observations
straight into device memory. With ``record=True`` the same kernel also
writes every env's episode as the contiguous ``[L + 4, 84, 84]`` plane
run that :meth:`DeviceFrameStackBuffer.store_frames
<machin_amd.frame.buffers.frame_stack_buffer.DeviceFrameStackBuffer.store_frames>`
stores, so an episode goes from env to replay without the host touching
a pixel.

Physics, clipping and rendering are those of ``PixelCatchEnv``; only
the random stream differs: a new ball's x comes from Philox4x32-10
keyed by the seed and counted by ``(ball number, env index)``, see
:func:`machin_amd.ops.pixelcatch_step`.
"""
from typing import Dict, List, Tuple, Union

import torch as t

from ... import ops
from ..wrappers.base import ParallelWrapperBase
from .classic_control import Space
from .pixel_catch import H, W

FRAMES = 4
STEPS_PER_BALL = 27  # ball_y runs 0, 3, .., 81: it lands on its 27th step


class DevicePixelCatchVecEnv(ParallelWrapperBase):
    """``num_envs`` PixelCatch envs stepped by one kernel launch.

    ``layout`` is ``"nchw"`` (``obs`` plain contiguous) or ``"nhwc"``
    (``obs`` in ``torch.channels_last`` strides, what the fused u8 conv
    stem and ``DeviceFrameStackBuffer(frame_layout="nhwc")`` use); the
    logical shape is ``[num_envs, 4, 84, 84]`` u8 either way, channel 3
    the newest frame.

    ``auto_reset=True`` resets an env inside the step that ends its
    episode: ``done`` is 1, ``info["frame"]`` is the terminal frame and
    ``obs`` already is the next episode's first state. With
    ``auto_reset=False`` a done env is latched until ``reset(idx)``:
    further steps return reward 0, done 1 and leave its ``obs`` alone.

    Actions outside ``{0, 1, 2}`` are CLAMPED into that range (the host
    env raises; a device env cannot look at values without waiting for
    the device).

    ``obs``, ``reward``, ``done`` and ``info["frame"]`` returned by
    :meth:`step` and :meth:`reset` are the env's own resident tensors:
    the next call rewrites them, so clone what must outlive it.
    ``step`` and ``reset`` never wait for the device.

    ``record=True`` keeps every env's running episode in HBM:
    ``num_envs * (max_len + 4) * 7056`` bytes of frames with ``max_len
    = min(max_episode_steps, 27 * balls)`` — 4 GB for 4096 envs at the
    defaults (``balls=5``: 139 planes per env) — plus 16 bytes per step
    for action, reward and terminal. See :meth:`finished_episodes`.

    On a CPU ``device`` the same semantics run as torch ops (slow; for
    tests and for trying code without a GPU).
    """

    def __init__(
        self,
        num_envs: int,
        device: Union[str, t.device] = "cuda:0",
        seed: int = 0,
        balls: int = 5,
        max_episode_steps: int = 1000,
        layout: str = "nchw",
        auto_reset: bool = True,
        record: bool = False,
    ):
        super().__init__()
        if int(num_envs) < 1:
            raise ValueError("num_envs must be at least 1.")
        if layout not in ("nchw", "nhwc"):
            raise ValueError("layout must be 'nchw' or 'nhwc'.")
        if int(balls) < 1 or int(max_episode_steps) < 1:
            raise ValueError(
                "balls and max_episode_steps must be at least 1."
            )
        self.num_envs = int(num_envs)
        self.device = t.device(device)
        self.balls = int(balls)
        self.max_episode_steps = int(max_episode_steps)
        self.layout = layout
        self.auto_reset = bool(auto_reset)
        self.record = bool(record)
        self.max_len = min(self.max_episode_steps,
                           STEPS_PER_BALL * self.balls)
        self._observation_space = Space(shape=(FRAMES, H, W))
        self._action_space = Space(n=3)

        E, dev = self.num_envs, self.device
        # every env starts latched: step() refuses to run before reset()
        self._state = t.zeros((E, 10), dtype=t.int32, device=dev)
        self._state[:, 5] = 1
        self._ball_no = t.zeros(E, dtype=t.int64, device=dev)
        if layout == "nhwc":
            # channels_last strides, also for a single env
            self._obs = t.zeros((E, H, W, FRAMES), dtype=t.uint8,
                                device=dev).permute(0, 3, 1, 2)
        else:
            self._obs = t.zeros((E, FRAMES, H, W), dtype=t.uint8,
                                device=dev)
        self._frame = t.zeros((E, H, W), dtype=t.uint8, device=dev)
        self._reward = t.zeros(E, dtype=t.float32, device=dev)
        self._done = t.zeros(E, dtype=t.float32, device=dev)
        self._ep_len = t.zeros(E, dtype=t.int32, device=dev)
        self._mask = t.zeros(E, dtype=t.uint8, device=dev)
        self._log = None
        if self.record:
            n = self.max_len
            self._log = (
                t.zeros((E, n + FRAMES, H, W), dtype=t.uint8, device=dev),
                t.zeros((E, n), dtype=t.int64, device=dev),
                t.zeros((E, n), dtype=t.float32, device=dev),
                t.zeros((E, n), dtype=t.float32, device=dev),
            )
        self._seed = 0
        self._was_reset = False
        self._closed = False
        self.seed(seed)

    # -- named views of the per-env state (flat device tensors) --------
    @property
    def paddle_x(self) -> t.Tensor:
        return self._state[:, 0]

    @property
    def ball_x(self) -> t.Tensor:
        return self._state[:, 1]

    @property
    def ball_y(self) -> t.Tensor:
        return self._state[:, 2]

    @property
    def balls_left(self) -> t.Tensor:
        return self._state[:, 3]

    @property
    def steps(self) -> t.Tensor:
        return self._state[:, 4]

    @property
    def done(self) -> t.Tensor:
        """Latched done flag (only ever set with ``auto_reset=False``)."""
        return self._state[:, 5]

    @property
    def history(self) -> t.Tensor:
        """``[E, 4]`` packed ``paddle_x | ball_x << 8 | ball_y << 16 |
        valid << 24``, newest last."""
        return self._state[:, 6:]

    @property
    def ball_no(self) -> t.Tensor:
        return self._ball_no

    # -- protocol ------------------------------------------------------
    def seed(self, seed=None) -> List[int]:
        """Set the Philox key and zero every env's ball counter, so the
        same seed replays the same balls. ``None`` means 0."""
        self._seed = (0 if seed is None else int(seed)) & (2 ** 64 - 1)
        self._ball_no.zero_()
        return [self._seed]

    def reset(self, idx=None) -> t.Tensor:
        """Reset all envs (``idx=None``) or those in an index list or
        an int64 index tensor; returns the resident ``obs``."""
        self._check_open()
        if idx is None:
            self._mask.fill_(1)
        else:
            if not t.is_tensor(idx):
                idx = t.as_tensor(list(idx), dtype=t.int64)
                if idx.numel() and not (
                    0 <= int(idx.min()) and int(idx.max()) < self.num_envs
                ):
                    raise ValueError("env index out of range.")
            elif idx.dtype != t.int64:
                raise ValueError("an index tensor must be int64.")
            # an index tensor's values are never looked at on the host;
            # out-of-range entries are ignored rather than addressed
            idx = idx.to(self.device, non_blocking=True).view(-1)
            inside = (idx >= 0) & (idx < self.num_envs)
            hits = t.zeros(self.num_envs, dtype=t.int32, device=self.device)
            hits.index_put_((idx.clamp(0, self.num_envs - 1),),
                            inside.int(), accumulate=True)
            self._mask.copy_(hits > 0)
        ops.pixelcatch_reset(self._state, self._ball_no, self._mask,
                             self._obs, self._seed, self.balls)
        self._was_reset = True
        return self._obs

    def step(self, action: t.Tensor, idx=None
             ) -> Tuple[t.Tensor, t.Tensor, t.Tensor, Dict[str, t.Tensor]]:
        """Step every env. ``action`` is an integer tensor on the env's
        device, ``[E]`` or ``[E, 1]``. Returns ``(obs, reward, done,
        info)`` with ``reward`` / ``done`` f32 ``[E]`` and
        ``info["frame"]`` the ``[E, 84, 84]`` newest plane of this
        step's next_state. All four are resident tensors rewritten by
        the next call. Does not wait for the device."""
        self._check_open()
        if idx is not None:
            raise ValueError(
                "DevicePixelCatchVecEnv steps all envs at once."
            )
        if not self._was_reset:
            raise RuntimeError("call reset() before step().")
        E = self.num_envs
        if not t.is_tensor(action):
            raise ValueError("action must be a tensor on the env's device.")
        if action.device != self.device:
            raise ValueError(
                f"action is on {action.device}, the env on {self.device}."
            )
        if action.dtype not in (t.int64, t.int32, t.int16, t.int8, t.uint8):
            raise ValueError("action must be an integer tensor.")
        if tuple(action.shape) not in ((E,), (E, 1)):
            raise ValueError(f"action must be [{E}] or [{E}, 1].")
        action = action.reshape(E).long().contiguous()
        ops.pixelcatch_step(
            self._state, self._ball_no, action, self._obs, self._frame,
            self._reward, self._done, self._ep_len, self._seed, self.balls,
            self.max_episode_steps, self.auto_reset, self._log,
        )
        return self._obs, self._reward, self._done, {"frame": self._frame}

    def finished_episodes(self):
        """Episodes that ended in the last :meth:`step` (``record=True``
        only): one ``(frames [L + 4, 84, 84] u8, {"action": [L, 1]
        int64, "reward": [L] f32, "terminal": [L] f32})`` tuple per
        such env, in env order. ``frames`` is what
        ``DeviceFrameStackBuffer.store_frames`` takes (the four planes
        of the first state, then every step's newest plane); the action
        is the clamped one.

        Everything returned is a VIEW of the env's log, valid until the
        next :meth:`step`. Reads one ``[E]`` tensor back (the lengths
        of the episodes that ended, 0 elsewhere): the only wait for the
        device in this class besides :meth:`active`."""
        if self._log is None:
            raise RuntimeError("finished_episodes() needs record=True.")
        frames, action, reward, terminal = self._log
        out = []
        for e, length in enumerate(self._ep_len.tolist()):
            if length <= 0:
                continue
            n = min(length, self.max_len)
            out.append((
                frames[e, : n + FRAMES],
                {
                    "action": action[e, :n].view(n, 1),
                    "reward": reward[e, :n],
                    "terminal": terminal[e, :n],
                },
            ))
        return out

    def active(self) -> List[int]:
        """Indices of the envs that are not done. Waits for the device
        (reads the latched flags back)."""
        return (self._state[:, 5] == 0).nonzero().view(-1).tolist()

    def size(self) -> int:
        return self.num_envs

    def render(self, idx=None, *_, **__) -> t.Tensor:
        """Newest plane of every env (or of ``idx``), from ``obs``."""
        newest = self._obs[:, -1]
        return newest if idx is None else newest[idx]

    def close(self) -> None:
        """Free the device tensors."""
        self._closed = True
        self._log = None
        self._obs = self._frame = None

    def _check_open(self):
        if self._closed:
            raise RuntimeError("the env is closed.")

    @property
    def action_space(self):
        return self._action_space

    @property
    def observation_space(self):
        return self._observation_space
