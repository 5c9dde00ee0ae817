"""Frame-deduplicated HBM replay fed one VECTOR STEP at a time.

No reference counterpart. :class:`.frame_stack_buffer.DeviceFrameStackBuffer`
takes whole episodes: a producer that steps thousands of device envs
has to find out on the host which episodes ended (a wait for the
device) and store each of them with a handful of small launches. This
buffer takes one step of ALL envs per call instead
(:meth:`DeviceVecFrameStackBuffer.append_step`): one gfx950 kernel
(:func:`machin_amd.ops.framestack_vec_append`) writes every env's newest
plane and does all the bookkeeping on the device, so storing never looks
at a value on the host.

Layout, with ``E = num_lanes``, ``S = lane_slots``, ``k = frame_stack``,
``n = n_step``, ``G = k + n`` and row stride ``R = S + G``:

* every env owns a *lane*: a ring of ``S`` plane slots that lays its
  episodes out the way ``DeviceFrameStackBuffer`` does (an episode of
  ``L`` transitions is ``L + k`` consecutive slots, transition ``t`` has
  its base at the episode's slot ``t``), followed by a MIRROR of the
  lane's first ``G`` slots. Everything written to slot ``i < G`` is also
  written to slot ``S + i``, so a window that starts near the end of a
  lane runs on into the mirror and never wraps;
* ``planes`` u8 ``[E*R, H, W]``, ``reward`` / ``terminal`` f32 ``[E*R]``,
  ``left`` int64 ``[E*R]`` and ``action`` ``[E*R, ...]`` are flat over
  all lanes, and a transition's position is its base plane slot. That
  is exactly the flat ring the existing gathers read
  (:func:`machin_amd.ops.framestack_gather` with ``base = pos``,
  :func:`machin_amd.ops.framestack_gather_nstep` with ``base =
  arange``), so sampling uses them unchanged;
* ``head`` / ``run`` int64 ``[E]``: planes a lane has written and the
  transitions of its running episode;
* one :class:`machin_amd.ops.sumtree.DeviceSumTree` over the ``E*R``
  positions holds the weight of every SAMPLEABLE transition (priority,
  or 1 when not prioritized) and 0 everywhere else. Mirror slots are
  never anyone's position, their leaves stay 0.

A transition is sampleable from the step that completes its n-step
window (or ends its episode) until its base plane is overwritten.
"""
from typing import Union

import torch as t

from ... import ops
from ...ops.sumtree import DeviceSumTree
from .device_buffer import DeviceTransitionBuffer


class DeviceVecFrameStackBuffer(DeviceTransitionBuffer):
    """Per-lane frame rings stored one vector step at a time.

    Protocol::

        buffer.begin(env.reset())                     # [E, k, H, W] u8
        obs, reward, done, info = env.step(action)
        buffer.append_step(action, reward, done, info["frame"], obs)

    with an auto-resetting env such as ``DevicePixelCatchVecEnv``:
    ``info["frame"]`` is the newest plane of the step's next_state (the
    terminal frame included) and ``obs`` already is the next episode's
    first state for the envs whose episode ended. ``begin`` and
    ``append_step`` never read from the device.

    ``lane_slots`` is the capacity of ONE lane in frames; it must be at
    least ``2 * (frame_stack + n_step)``. An episode of ``L``
    transitions costs ``L + k`` slots, as in ``DeviceFrameStackBuffer``.
    The buffer allocates ``num_lanes * (lane_slots + k + n) * H * W``
    bytes of planes at :meth:`begin`.

    :meth:`sample_batch` has the signature and the return structure of
    ``DeviceFrameStackBuffer.sample_batch`` (``frame_layout``,
    ``n_step``, ``discount`` and ``augment_shift`` mean the same, and
    the ``n_step`` / ``shift`` attributes come back under ``"*"``), so
    RAINBOW, DQN and DQNPer take the buffer through ``replay_buffer=``.
    Uniform draws (``prioritized=False``) are non-stratified draws from
    the tree of unit weights; prioritized draws are stratified, with
    importance weights ``(p / min p) ** -beta`` over the batch (the
    number of live transitions cancels in that normalisation, so none is
    needed). New transitions get the running maximum priority.

    Known limit: with ``prioritized=False`` the tree sums ones in
    float32, which is exact only up to ``2 ** 24`` sampleable
    transitions.

    ``store_episode`` / ``store_transition`` / ``store_frames`` do not
    exist here: a lane ring is filled by :meth:`append_step` only.
    """

    def __init__(
        self,
        num_lanes: int,
        lane_slots: int,
        device: Union[str, t.device] = "cuda:0",
        frame_stack: int = 4,
        frame_key: str = "state",
        frame_layout: str = "nchw",
        prioritized: bool = False,
        n_step: int = 1,
        discount: float = 0.99,
        augment_shift: int = 0,
        **per_kwargs,
    ):
        self.num_lanes = int(num_lanes)
        self.lane_slots = int(lane_slots)
        if self.num_lanes < 1:
            raise ValueError("num_lanes must be at least 1.")
        super().__init__(
            self.num_lanes * max(self.lane_slots, 0), device, prioritized,
            **per_kwargs,
        )
        self.augment_shift = int(augment_shift)
        if not 0 <= self.augment_shift <= 16:
            raise ValueError("augment_shift must be in [0, 16].")
        self.frame_stack = int(frame_stack)
        if not 1 <= self.frame_stack <= 8:
            raise ValueError("frame_stack must be in [1, 8].")
        self.n_step = int(n_step)
        if not 1 <= self.n_step <= 16:
            raise ValueError("n_step must be in [1, 16].")
        self.discount = float(discount)
        self._mirror = self.frame_stack + self.n_step
        if self.lane_slots < 2 * self._mirror:
            raise ValueError(
                "lane_slots must be at least 2 * (frame_stack + n_step)."
            )
        if frame_layout not in ("nchw", "nhwc"):
            raise ValueError("frame_layout must be 'nchw' or 'nhwc'.")
        self.frame_key = frame_key
        self.frame_layout = frame_layout
        self.epsilon = self._per_kwargs["epsilon"]
        self.alpha = self._per_kwargs["alpha"]
        self.curr_beta = self._per_kwargs["beta"]
        self.beta_increment_per_sampling = self._per_kwargs[
            "beta_increment_per_sampling"
        ]
        self._state_col = f"state/{frame_key}"
        self._next_col = f"next_state/{frame_key}"
        self._attr_order = ["action", "next_state", "reward", "state",
                            "terminal"]
        self._row = self.lane_slots + self._mirror
        dev = self.buffer_device
        rows = self.num_lanes * self._row
        self._planes = None  # [E*R, H, W] u8, allocated by begin()
        self._action = None  # [E*R, ...], allocated by the first step
        self._reward = t.zeros(rows, dtype=t.float32, device=dev)
        self._terminal = t.zeros(rows, dtype=t.float32, device=dev)
        self._left = t.zeros(rows, dtype=t.int64, device=dev)
        # a transition's base plane slot is its own position
        self._base = t.arange(rows, dtype=t.int64, device=dev)
        self._lane = t.arange(self.num_lanes, dtype=t.int64,
                              device=dev) * self._row
        self._head = t.zeros(self.num_lanes, dtype=t.int64, device=dev)
        self._run = t.zeros(self.num_lanes, dtype=t.int64, device=dev)
        self._tree = DeviceSumTree(rows, dev)
        self._one = t.ones((), dtype=t.float32, device=dev)
        self._max_priority = t.ones((), dtype=t.float32, device=dev)
        self._begun = False
        self.steps_stored = 0  # host counter: append_step calls

    # -- storing -------------------------------------------------------
    def _check_stack(self, name: str, obs: t.Tensor):
        E, k = self.num_lanes, self.frame_stack
        if not t.is_tensor(obs) or obs.dtype != t.uint8:
            raise ValueError(f"{name} must be a uint8 tensor.")
        if obs.dim() != 4 or obs.shape[0] != E or obs.shape[1] != k:
            raise ValueError(
                f"{name} must be [{E}, {k}, H, W], got {list(obs.shape)}."
            )
        if obs.device != self.buffer_device:
            raise ValueError(
                f"{name} is on {obs.device}, the buffer on "
                f"{self.buffer_device}."
            )
        if self._planes is not None \
                and obs.shape[2:] != self._planes.shape[1:]:
            raise ValueError("Frame size differs from the ring's.")

    def begin(self, obs: t.Tensor):
        """Start a new episode in every lane from ``obs`` (u8
        ``[E, k, H, W]``, what ``env.reset()`` returns): writes each
        lane's first state at its head. Running episodes are abandoned;
        their incomplete windows never become sampleable. Torch ops, no
        host read; meant to run once per reset of all envs."""
        self._check_stack("obs", obs)
        E, S, G = self.num_lanes, self.lane_slots, self._mirror
        with self._lock:
            if self._planes is None:
                self._planes = t.zeros(
                    (E * self._row, *obs.shape[2:]), dtype=t.uint8,
                    device=self.buffer_device,
                )
            dead = []
            for j in range(self.frame_stack):
                slot = (self._head + j) % S
                idx = self._lane + slot
                plane = obs[:, j]
                self._planes.index_copy_(0, idx, plane)
                # the mirror; lanes without one write the slot again
                self._planes.index_copy_(
                    0, t.where(slot < G, idx + S, idx), plane
                )
                dead.append(idx)
            dead = t.cat(dead)
            self._tree.update_leaf_batch(
                t.zeros(dead.numel(), device=self.buffer_device), dead
            )
            self._head += self.frame_stack
            self._run.zero_()
            self._begun = True

    def append_step(self, action: t.Tensor, reward: t.Tensor,
                    done: t.Tensor, frame: t.Tensor, next_obs: t.Tensor,
                    terminal: t.Tensor = None):
        """Store one step of all ``E`` envs.

        ``action`` is ``[E]`` or ``[E, ...]`` (the first one stored
        fixes dtype and shape), ``reward`` and ``done`` f32 ``[E]``,
        ``frame`` u8 ``[E, H, W]`` the newest plane of the step's
        next_state, ``next_obs`` u8 ``[E, k, H, W]`` (contiguous or
        ``channels_last``) the observation after the step, read only
        for the lanes with ``done != 0`` as their next episode's first
        state. ``terminal`` (f32 ``[E]``, default ``done``) is what is
        stored as the transition's terminal flag; it differs from
        ``done`` for an episode cut by a time limit.

        One :func:`machin_amd.ops.framestack_vec_append`, one
        ``index_copy_`` of the action and one sum-tree update; never
        reads from the device."""
        if not self._begun:
            raise RuntimeError("call begin() before append_step().")
        E = self.num_lanes
        self._check_stack("next_obs", next_obs)
        if not t.is_tensor(action) or action.dim() < 1 \
                or action.shape[0] != E:
            raise ValueError(f"action must be a tensor with {E} rows.")
        if action.device != self.buffer_device:
            raise ValueError(
                f"action is on {action.device}, the buffer on "
                f"{self.buffer_device}."
            )
        if action.dim() == 1:
            action = action.view(E, 1)
        if terminal is None:
            terminal = done
        with self._lock:
            if self._action is None:
                self._action = t.zeros(
                    (E * self._row, *action.shape[1:]), dtype=action.dtype,
                    device=self.buffer_device,
                )
            elif action.dtype != self._action.dtype \
                    or action.shape[1:] != self._action.shape[1:]:
                raise ValueError(
                    f"action must be {self._action.dtype} "
                    f"[{E}, {', '.join(map(str, self._action.shape[1:]))}]"
                    f" like the first one stored."
                )
            fill = self._max_priority if self.prioritized else self._one
            pos, leaf_idx, leaf_w = ops.framestack_vec_append(
                self._planes, self._reward, self._terminal, self._left,
                self._head, self._run, frame, next_obs, reward, terminal,
                done, fill, self.frame_stack, self.n_step,
            )
            self._action.index_copy_(0, pos, action)
            self._tree.update_leaf_batch(leaf_w.view(-1), leaf_idx.view(-1))
            self.steps_stored += 1

    def _refuse(self, name):
        raise NotImplementedError(
            f"DeviceVecFrameStackBuffer has no {name}: it stores one step "
            f"of all lanes at a time, use append_step."
        )

    def store_episode(self, *_, **__):
        self._refuse("store_episode")

    def store_transition(self, *_, **__):
        self._refuse("store_transition")

    append = store_transition

    def store_frames(self, *_, **__):
        self._refuse("store_frames")

    def store_flat(self, *_, **__):
        self._refuse("store_flat")

    # -- sampling ------------------------------------------------------
    def sample_batch(
        self,
        batch_size: int,
        concatenate: bool = True,
        device=None,
        sample_method=None,
        sample_attrs=None,
        additional_concat_custom_attrs=None,
        *_,
        **__,
    ):
        if not concatenate:
            raise ValueError(
                "DeviceVecFrameStackBuffer only supports concatenated "
                "sampling (flat device rings)."
            )
        with self._lock:
            # after n_step steps every lane holds a sampleable transition
            if self.steps_stored < self.n_step or batch_size <= 0:
                return (0, None, None, None) if self.prioritized \
                    else (0, None)
            pos = self._tree.sample(batch_size,
                                    stratified=self.prioritized)
            # find_leaf_index never returns a zero leaf while the tree
            # holds weight; should it, take another position of the batch
            leaf_w = self._tree.get_leaf_weight(pos)
            good = leaf_w > 0
            spare = pos.index_select(
                0, good.to(t.uint8).argmax().view(1)
            )
            pos = t.where(good, pos, spare)
            is_weight = None
            if self.prioritized:
                leaf_w = self._tree.get_leaf_weight(pos).clamp_min(1e-30)
                is_weight = (leaf_w / leaf_w.min()) ** (-self.curr_beta)
                self.curr_beta = min(
                    1.0,
                    self.curr_beta + self.beta_increment_per_sampling,
                )
            shift = None
            if self.augment_shift > 0:
                pad = self.augment_shift
                shift = t.randint(
                    -pad, pad + 1, (batch_size, 4), dtype=t.int32,
                    device=self.buffer_device,
                )
            cols = {"action/action": self._action.index_select(0, pos)}
            nhwc = self.frame_layout == "nhwc"
            if self.n_step > 1:
                (
                    state, next_state, cols["reward"], cols["terminal"],
                    steps,
                ) = ops.framestack_gather_nstep(
                    self._planes, self._base, self._left, self._reward,
                    self._terminal, pos, self.frame_stack, self.n_step,
                    self.discount, channels_last=nhwc, shift=shift,
                )
                cols["n_step"] = steps.view(-1, 1)
            else:
                cols["reward"] = self._reward.index_select(0, pos)
                cols["terminal"] = self._terminal.index_select(0, pos)
                state, next_state = ops.framestack_gather(
                    self._planes, pos, self.frame_stack,
                    channels_last=nhwc, shift=shift,
                )
            if shift is not None:
                cols["shift"] = shift
            cols[self._state_col] = state
            cols[self._next_col] = next_state
            attrs = sample_attrs or (self._attr_order + ["*"])
            batch = self._structure(cols, attrs)
            if self.prioritized:
                return batch_size, batch, pos, is_weight
            return batch_size, batch

    # -- PER interface -------------------------------------------------
    def update_priority(self, priorities, indexes):
        if not self.prioritized:
            raise RuntimeError("Buffer is not prioritized.")
        dev = self.buffer_device
        with self._lock:
            prio = t.as_tensor(priorities, dtype=t.float32).to(dev)
            pos = t.as_tensor(indexes).to(dev).long().view(-1)
            prio = (prio.view(-1).abs() + self.epsilon) ** self.alpha
            # a position overwritten since it was sampled stays at 0
            live = self._tree.get_leaf_weight(pos) > 0
            prio = t.where(live, prio, t.zeros_like(prio))
            self._max_priority = t.maximum(
                self._max_priority, prio.max()
            )
            self._tree.update_leaf_batch(prio, pos)

    # -- bookkeeping ---------------------------------------------------
    def size(self) -> int:
        """Exact number of sampleable transitions. Waits for the device
        (counts the positive leaves and reads the count back); use
        :attr:`steps_stored` in loop conditions that must not wait."""
        return int((self._tree.get_leaf_all_weights() > 0).sum().item())

    def clear(self):
        with self._lock:
            self._head.zero_()
            self._run.zero_()
            self._left.zero_()
            self._tree.weights.zero_()
            self._max_priority = t.ones(
                (), dtype=t.float32, device=self.buffer_device
            )
            self.curr_beta = self._per_kwargs["beta"]
            self._begun = False
            self.steps_stored = 0
