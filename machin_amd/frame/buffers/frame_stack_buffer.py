"""Frame-deduplicated HBM replay for frame-stacked pixel observations.

No reference counterpart. :class:`.device_buffer.DeviceTransitionBuffer`
stores each Atari-shaped transition as two full ``[4, 84, 84]`` u8
stacks (``state`` and ``next_state``): 56 448 bytes for 7 056 bytes of
new information, because seven of the eight planes are copies of planes
held by neighbouring transitions. This buffer stores every frame ONCE
in a ring of planes and rebuilds both stacks when sampling with one
gfx950 kernel (:func:`machin_amd.ops.framestack_gather`), so the same
HBM holds about eight times as many transitions.

Layout:

* frame ring ``[buffer_size, H, W]`` u8 — an episode of ``L``
  transitions occupies ``L + k`` consecutive slots: the ``k`` planes
  of its first state, then the newest plane of every next_state;
* transition ring — every other column (other state keys, action,
  reward, terminal, custom attributes) plus one int64 column holding
  the transition's base plane slot. Transition ``t`` of an episode
  written at slot ``s`` has base ``s + t``; its state is planes
  ``base .. base+k-1`` and its next_state planes ``base+1 .. base+k``.

With ``n_step > 1`` the transition ring also holds the number of
transitions left in the episode, and sampling uses
:func:`machin_amd.ops.framestack_gather_nstep`, which folds RAINBOW's
n-step reward / terminal / ``next_state = state_{t+m}`` from the raw
1-step rows in the same kernel (see the class docstring).

Eviction is by overwritten planes. All bookkeeping is host integers
(absolute plane / transition counters and a deque of ``(first base,
count)`` per episode), so neither storing nor sampling waits for the
device.
"""
from collections import deque
from typing import Dict, Union

import torch as t

from ... import ops
from .device_buffer import DeviceReplayBuffer, DeviceTransitionBuffer


class DeviceFrameStackBuffer(DeviceTransitionBuffer):
    """Device replay that stores each frame once.

    Speaks the algorithm-facing API of :class:`DeviceTransitionBuffer`
    (``store_episode`` / ``store_transition`` / ``sample_batch`` /
    ``update_priority`` / ``size`` / ``clear``), so any algorithm takes
    it through its ``replay_buffer=`` argument. :meth:`store_frames` is
    the tensor path of ``store_episode`` for producers that already hold
    an episode as a plane run (``DevicePixelCatchVecEnv(record=True)``).

    ``buffer_size`` is the capacity in FRAMES (ring planes), not in
    transitions: an episode of ``L`` transitions costs ``L + k`` slots,
    so at most ``buffer_size - k`` transitions are live. A transition
    stored alone (``store_transition``) is an episode of length 1 and
    costs ``k + 1`` slots — store whole episodes to get the saving.

    ``state[frame_key]`` / ``next_state[frame_key]`` must be u8
    ``[1, k, H, W]`` sliding-window stacks: within an episode
    ``next_state_t[:k-1] == state_t[1:]`` and ``state_{t+1} ==
    next_state_t``. With ``validate=True`` this is checked on every
    ``store_episode`` (for frames that already live on a GPU the check
    reads one flag back, the only host wait in this class; keep frames
    on the host or pass ``validate=False`` to avoid it). Whatever
    padding the environment used at reset is kept bit-for-bit because
    the first state's ``k`` planes are stored as they are.

    ``frame_layout="nhwc"`` returns the sampled stacks in
    ``torch.channels_last`` strides (logical shape stays
    ``[B, k, H, W]``).

    Eviction: writing ring slots ``[h, h+n)`` kills exactly the
    transitions whose base lies in that range (windows look forward and
    never leave their own episode's slots), oldest first, so live
    transitions stay a contiguous range of the transition ring.

    ``n_step > 1`` (at most 16) turns on n-step sampling for RAINBOW:
    episodes are still stored RAW, one step per transition, plus one
    int64 column with the number of transitions left in the episode,
    and :func:`machin_amd.ops.framestack_gather_nstep` folds the
    n-step return when sampling. A sampled transition ``t`` with
    ``m = min(n_step, L - t)`` comes back with ``reward = sum_{j<m}
    discount^j r_{t+j}`` (cut at a terminal), ``terminal = max_{j<m}
    terminal_{t+j}``, ``next_state = state_{t+m}`` and the custom
    attribute ``n_step = m`` (``[B, 1]`` int64, under ``"*"``) — the
    rows RAINBOW's host fold would have stored. ``reward`` and
    ``terminal`` must be scalar float32 columns.

    Eviction, priorities and ``size()`` are the same for every
    ``n_step``: a window only looks FORWARD, at the ``m + k`` planes
    from its base on (inside the episode's ``L + k`` slots, since
    ``t + m <= L``) and at the next ``m - 1`` transitions of its own
    episode. Planes and transitions are both overwritten oldest first,
    so everything a live transition's window needs was written after
    its base plane and outlives it.

    ``augment_shift = pad`` (1 to 16; 0, the default, is off) applies
    the random shift of DrQ / RAD / data-efficient Rainbow to every
    sampled batch: replicate-pad by ``pad`` and crop back at a random
    offset, drawn independently for ``state`` and ``next_state`` and
    shared by the ``k`` planes of a stack. Each ``sample_batch`` draws
    one int32 ``[B, 4]`` tensor ``(dy_state, dx_state, dy_next,
    dx_next)``, uniform on ``[-pad, pad]``, on the buffer's device from
    that device's default generator (``t.manual_seed`` reproduces it; no
    host read), and passes it as ``shift=`` to the gather op, so the
    augmentation costs no extra pass over the pixels. The tensor comes
    back as the custom attribute ``shift`` (under ``"*"``). Storing,
    eviction, priorities and ``size()`` are unchanged and the ring
    always holds the original frames. With ``augment_shift=0`` sampling
    launches nothing more and returns no ``shift`` attribute.
    """

    def __init__(
        self,
        buffer_size: int,
        device: Union[str, t.device] = "cuda:0",
        frame_stack: int = 4,
        frame_key: str = "state",
        frame_layout: str = "nchw",
        prioritized: bool = False,
        validate: bool = True,
        n_step: int = 1,
        discount: float = 0.99,
        augment_shift: int = 0,
        **per_kwargs,
    ):
        super().__init__(buffer_size, device, prioritized, **per_kwargs)
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
        if self.buffer_size < self.frame_stack + self.n_step:
            raise ValueError(
                "buffer_size (frames) must be at least frame_stack + "
                "n_step."
            )
        if frame_layout not in ("nchw", "nhwc"):
            raise ValueError("frame_layout must be 'nchw' or 'nhwc'.")
        self.frame_key = frame_key
        self.frame_layout = frame_layout
        self.validate = validate
        self.epsilon = self._per_kwargs["epsilon"]
        self.alpha = self._per_kwargs["alpha"]
        self.curr_beta = self._per_kwargs["beta"]
        self.beta_increment_per_sampling = self._per_kwargs[
            "beta_increment_per_sampling"
        ]
        self._state_col = f"state/{frame_key}"
        self._next_col = f"next_state/{frame_key}"
        # an episode wastes k slots, so this bounds the live count
        self._t_capacity = self.buffer_size - self.frame_stack
        self._planes = None  # [buffer_size, H, W] u8, first store
        self._tree = None
        self._max_priority = None
        self._reset_counters()

    def _reset_counters(self):
        self._plane_count = 0  # absolute: planes ever written
        self._t_count = 0  # absolute: transitions ever written
        self._live = 0
        # per episode [absolute first live base, live count], oldest first
        self._episodes = deque()

    # -- layout --------------------------------------------------------
    def _ensure_rings(self, cols: Dict[str, t.Tensor], frame_shape):
        if self._inner is not None:
            return
        dev = self.buffer_device
        spec = {
            k: (tuple(v.shape[1:]), v.dtype) for k, v in cols.items()
        }
        self._inner = DeviceReplayBuffer(self._t_capacity, spec, dev)
        self._planes = t.empty(
            (self.buffer_size, *frame_shape), dtype=t.uint8, device=dev
        )
        if self.prioritized:
            from ...ops.sumtree import DeviceSumTree

            self._tree = DeviceSumTree(self._t_capacity, dev)
            self._max_priority = t.ones((), device=dev)
        self._attr_order = sorted(
            {k.split("/", 1)[0] for k in spec
             if k not in ("_base", "_left")}
            | {"state", "next_state"}
        )

    def _check_frames(self, states: t.Tensor, nexts: t.Tensor):
        """Sliding-window property of an episode's [L, k, H, W] stacks."""
        bad = (nexts[:, :-1] != states[:, 1:]).flatten(1).any(1)
        if states.shape[0] > 1:
            bad[:-1] |= (states[1:] != nexts[:-1]).flatten(1).any(1)
        if bool(bad.any()):
            step = int(bad.nonzero()[0])
            raise ValueError(
                f"Frames of step {step} are not a sliding window: need "
                f"next_state[:k-1] == state[1:] and the following "
                f"state == next_state (pass validate=False to store "
                f"anyway)."
            )

    # -- storing -------------------------------------------------------
    def store_flat(self, batch):
        raise NotImplementedError(
            "DeviceFrameStackBuffer stores whole episodes "
            "(store_episode); a flat batch has no frame order."
        )

    def store_episode(self, episode, required_attrs=("state", "action",
                      "next_state", "reward", "terminal"), **__):
        k = self.frame_stack
        cols = self.flatten_episode(episode, required_attrs)
        if self._state_col not in cols or self._next_col not in cols:
            raise ValueError(
                f"Transitions need state[{self.frame_key!r}] and "
                f"next_state[{self.frame_key!r}] frame stacks."
            )
        states = cols.pop(self._state_col)
        nexts = cols.pop(self._next_col)
        for name, v in (("state", states), ("next_state", nexts)):
            if v.dtype != t.uint8 or v.dim() != 4 or v.shape[1] != k:
                raise ValueError(
                    f"{name}[{self.frame_key!r}] must be a uint8 "
                    f"[1, {k}, H, W] frame stack, got "
                    f"{tuple(v.shape[1:])} {v.dtype}."
                )
        if nexts.shape != states.shape:
            raise ValueError("state and next_state frame shapes differ.")
        self._check_fits(states.shape[0])
        if self.validate:
            self._check_frames(states, nexts)
        self._store_run(t.cat([states[0], nexts[:, -1]], dim=0), cols)

    def store_frames(self, frames: t.Tensor, columns: Dict[str, t.Tensor]):
        """The tensor path of :meth:`store_episode`: store one episode
        of ``L`` transitions given as the plane run the frame ring
        keeps.

        ``frames`` is u8 ``[L + k, H, W]``, on any device: the ``k``
        planes of the first state, then the newest plane of every
        next_state (transition ``i`` has state ``frames[i : i + k]`` and
        next_state ``frames[i + 1 : i + k + 1]``). ``columns`` maps the
        names :meth:`flatten_episode` produces — ``"action/action"``,
        ``"reward"``, ``"terminal"``, custom attributes, other
        ``"state/..."`` keys — to ``[L, ...]`` tensors, on any device.

        Eviction, priorities, counters and what sampling returns are
        those of ``store_episode`` with the same episode. There is no
        list of dicts, no sliding-window check (a plane run cannot
        violate it); an episode whose tensors are all on a GPU is stored
        with device copies only, without a host copy and without waiting
        for the device (host tensors go through the pinned slabs as in
        ``store_episode``)."""
        k = self.frame_stack
        if not t.is_tensor(frames) or frames.dtype != t.uint8 \
                or frames.dim() != 3 or frames.shape[0] <= k:
            raise ValueError(
                f"frames must be a uint8 [L + {k}, H, W] tensor with "
                f"L >= 1."
            )
        L = frames.shape[0] - k
        cols = {}
        for name, v in columns.items():
            if name in (self._state_col, self._next_col, "_base", "_left"):
                raise ValueError(f"Column {name!r} is made by the buffer.")
            if not t.is_tensor(v) or v.dim() < 1 or v.shape[0] != L:
                raise ValueError(
                    f"Column {name!r} must be a tensor with {L} rows."
                )
            cols[name] = v.detach()
        self._check_fits(L)
        self._store_run(frames.detach(), cols)

    def _check_fits(self, L: int):
        n = L + self.frame_stack
        if n > self.buffer_size:
            raise ValueError(
                f"Episode of {L} transitions needs {n} frame slots, "
                f"buffer_size is {self.buffer_size}."
            )

    def _store_run(self, frames: t.Tensor, cols: Dict[str, t.Tensor]):
        """Write one episode: its plane run ``[L + k, H, W]`` and its
        other columns ``[L, ...]`` (shared by :meth:`store_episode` and
        :meth:`store_frames`)."""
        L = frames.shape[0] - self.frame_stack
        n = frames.shape[0]
        with self._lock:
            F, T = self.buffer_size, self._t_capacity
            first = self._plane_count
            # index columns are born where the frames are: frames that
            # already live on a GPU bring no host tensor along
            idx_dev = frames.device if frames.is_cuda else None
            cols["_base"] = t.arange(first, first + L, dtype=t.int64,
                                     device=idx_dev) % F
            if self.n_step > 1:
                for name in ("reward", "terminal"):
                    v = cols.get(name)
                    if v is None or v.dim() != 1 or v.dtype != t.float32:
                        raise ValueError(
                            f"n_step > 1 needs {name!r} as a scalar "
                            f"float32 column."
                        )
                # transitions that follow in the episode
                cols["_left"] = t.arange(L - 1, -1, -1, dtype=t.int64,
                                         device=idx_dev)
            self._ensure_rings(cols, tuple(frames.shape[1:]))
            # refuse before any bookkeeping changes
            if frames.shape[1:] != self._planes.shape[1:]:
                raise ValueError("Frame size differs from the ring's.")
            if set(cols) != set(self._inner.spec):
                raise ValueError(
                    f"Transition attributes {sorted(cols)} differ from "
                    f"the stored ones {sorted(self._inner.spec)}."
                )
            # -- evict by overwritten planes (host integers only)
            t_tail = self._t_count - self._live
            horizon = first + n - F  # absolute bases below this die
            killed = 0
            while self._episodes and self._episodes[0][0] < horizon:
                ep = self._episodes[0]
                dead = min(ep[1], horizon - ep[0])
                ep[0] += dead
                ep[1] -= dead
                killed += dead
                if ep[1] == 0:
                    self._episodes.popleft()
            self._live -= killed
            # -- one H2D copy per host column through the pinned slabs
            # (an episode that is on a GPU already skips the slabs and
            # the wait for their previous copies)
            staged = {**cols, "_frames": frames}
            from_host = any(not v.is_cuda for v in staged.values())
            if from_host:
                staged = self._stage(staged)
            frames = staged.pop("_frames").to(
                self.buffer_device, non_blocking=True
            )
            h = first % F
            if h + n <= F:
                self._planes[h : h + n] = frames
            else:
                self._planes[h:] = frames[: F - h]
                self._planes[: h + n - F] = frames[F - h :]
            pos = self._inner.store_batch(staged)
            if from_host and self._pinned_event is not None:
                self._pinned_event.record()
            if self._tree is not None:
                # killed slots that the new transitions do not reuse
                # get priority 0; new ones the running max priority
                t_head = self._t_count
                lo = max(t_tail, t_head + L - T)
                dead_pos = t.arange(
                    lo, max(lo, t_tail + killed),
                    device=self.buffer_device,
                ) % T
                self._tree.update_leaf_batch(
                    t.cat([
                        t.zeros(dead_pos.numel(),
                                device=self.buffer_device),
                        self._max_priority.expand(L),
                    ]),
                    t.cat([dead_pos, pos]),
                )
            self._episodes.append([first, L])
            self._plane_count += n
            self._t_count += L
            self._live += L

    # -- sampling ------------------------------------------------------
    def _is_live(self, pos: t.Tensor) -> t.Tensor:
        tail = (self._t_count - self._live) % self._t_capacity
        return (pos - tail) % self._t_capacity < self._live

    def _uniform_live(self, batch_size: int) -> t.Tensor:
        tail = self._t_count - self._live
        return (
            t.randint(0, self._live, (batch_size,),
                      device=self.buffer_device) + tail
        ) % self._t_capacity

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
                "DeviceFrameStackBuffer only supports concatenated "
                "sampling (flat device rings)."
            )
        with self._lock:
            if self._live == 0 or batch_size <= 0:
                return (0, None, None, None) if self.prioritized \
                    else (0, None)
            is_weight = None
            if self.prioritized:
                pos = self._tree.sample(batch_size, stratified=True)
                # the float edge of the stratified search can land on
                # a zero-priority (dead) leaf: swap in a live one
                pos = t.where(
                    self._is_live(pos), pos,
                    self._uniform_live(batch_size),
                )
                leaf_w = self._tree.get_leaf_weight(pos)
                total = self._tree.get_weight_sum_tensor()
                probs = (leaf_w / total).clamp_min(1e-12)
                is_weight = (self._live * probs) ** (-self.curr_beta)
                is_weight = is_weight / is_weight.max()
                self.curr_beta = min(
                    1.0,
                    self.curr_beta + self.beta_increment_per_sampling,
                )
            else:
                pos = self._uniform_live(batch_size)
            shift = None
            if self.augment_shift > 0:
                pad = self.augment_shift
                shift = t.randint(
                    -pad, pad + 1, (batch_size, 4), dtype=t.int32,
                    device=self.buffer_device,
                )
            if self.n_step > 1:
                # the kernel indexes these four ring columns itself
                data = self._inner.data
                fused = ("_base", "_left", "reward", "terminal")
                cols = {
                    k: buf.index_select(0, pos)
                    for k, buf in data.items() if k not in fused
                }
                (
                    state, next_state, cols["reward"], cols["terminal"],
                    steps,
                ) = ops.framestack_gather_nstep(
                    self._planes, *(data[k] for k in fused), pos,
                    self.frame_stack, self.n_step, self.discount,
                    channels_last=self.frame_layout == "nhwc",
                    shift=shift,
                )
                cols["n_step"] = steps.view(-1, 1)
            else:
                cols = self._inner.gather(pos)
                state, next_state = ops.framestack_gather(
                    self._planes, cols.pop("_base"), self.frame_stack,
                    channels_last=self.frame_layout == "nhwc",
                    shift=shift,
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
        if self._tree is None:
            raise RuntimeError("Buffer is not prioritized (or empty).")
        dev = self.buffer_device
        with self._lock:
            prio = t.as_tensor(priorities, dtype=t.float32).to(dev)
            pos = t.as_tensor(indexes).to(dev).long().view(-1)
            prio = (prio.view(-1).abs() + self.epsilon) ** self.alpha
            # a slot evicted since it was sampled stays at priority 0
            prio = t.where(self._is_live(pos), prio, t.zeros_like(prio))
            self._max_priority = t.maximum(
                self._max_priority, prio.max()
            )
            self._tree.update_leaf_batch(prio, pos)

    # -- bookkeeping ---------------------------------------------------
    def size(self) -> int:
        """Number of live transitions."""
        return self._live

    def clear(self):
        with self._lock:
            self._reset_counters()
            self.curr_beta = self._per_kwargs["beta"]
            if self._inner is not None:
                self._inner.clear()
            if self._tree is not None:
                self._tree.weights.zero_()
                self._max_priority = t.ones((), device=self.buffer_device)
