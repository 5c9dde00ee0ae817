"""Shared helpers for the n-step frame-stack tests: the per-sample loop
that defines ``ops.framestack_gather_nstep`` (reward in float64), the
op cases, the host-fold oracle (RAINBOW's unchanged ``store_episode``
fold into a plain ``DeviceTransitionBuffer``), a plain-python liveness
model of the plane ring and the wrap/eviction round trip run on CPU and
on the GPU. Nothing here calls the code under test to get a reference.
"""
import functools
from types import SimpleNamespace

import torch as t

from util_framestack import K, H, W, LENGTHS

P_RING, T_RING, BATCH = 13, 11, 37
N_STEPS = [1, 2, 3, 5]


# -- op oracle -----------------------------------------------------------
def loop_reference(planes, base, left, reward, terminal, pos, k, n, gamma):
    """Literal per-sample definition of the op, python integers for the
    indices and float64 for the reward. Also returns the reward bound
    ``n * 2^-23 * sum_j gamma^j |r_j|`` of each sample."""
    n_planes, n_rows = planes.shape[0], len(base)
    base, left, pos = base.tolist(), left.tolist(), pos.tolist()
    reward, terminal = reward.double().tolist(), terminal.tolist()
    batch = len(pos)
    state = t.empty((batch, k, *planes.shape[1:]), dtype=t.uint8)
    next_state = t.empty_like(state)
    reward_n = t.empty(batch, dtype=t.float64)
    bound = t.empty(batch, dtype=t.float64)
    terminal_n = t.empty(batch, dtype=t.float32)
    steps = t.empty(batch, dtype=t.int64)
    for b in range(batch):
        p = pos[b] % n_rows
        s = base[p] % n_planes
        m = min(n, min(max(left[p], 0), n - 1) + 1)
        acc, mag, alive, term = 0.0, 0.0, 1.0, 0.0
        for j in range(m):
            q = (p + j) % n_rows
            acc += gamma ** j * reward[q] * alive
            mag += gamma ** j * abs(reward[q])
            alive *= 1.0 - terminal[q]
            term = max(term, terminal[q])
        reward_n[b], bound[b] = acc, n * 2.0 ** -23 * mag
        terminal_n[b], steps[b] = term, m
        for j in range(k):
            state[b, j] = planes[(s + j) % n_planes]
            next_state[b, j] = planes[(s + m + j) % n_planes]
    return state, next_state, reward_n, bound, terminal_n, steps


@functools.lru_cache(maxsize=None)
def op_inputs(h, w, kind, p_ring=P_RING, t_ring=T_RING, batch=BATCH):
    """Ring columns and sampled positions of one op case (do not
    modify: cached and shared). Both rings wrap; ``pos``, ``base`` and
    ``left`` carry negative and far out-of-range entries.

    The transition ring holds two episodes: rows 8,9,10,0,1,2 and rows
    3..7, so ``left`` covers 0..5 and a window wraps the ring's end.
    Terminals sit at both episode ends and at rows 5 and 9, i.e. at
    the first, a middle and the last step of some window for every n.
    ``kind`` is ``"exact"`` (small integer rewards, gamma 0.5: every
    partial sum is exact in fp32) or ``"random"`` (fp32 normal rewards,
    gamma 0.99)."""
    gen = t.Generator().manual_seed(h * 1000 + w)
    planes = t.randint(0, 256, (p_ring, h, w), dtype=t.uint8,
                       generator=gen)
    base = t.randint(0, p_ring, (t_ring,), generator=gen)
    pos = t.randint(0, t_ring, (batch,), generator=gen)
    if t_ring == T_RING:
        left = t.tensor([2, 1, 0, 4, 3, 2, 1, 0, 5, 4, 3])
        terminal = t.zeros(t_ring)
        terminal[[2, 5, 7, 9]] = 1.0
        # out-of-range values: the op reduces / clamps them itself
        left[0], left[10] = -5, 2 ** 40
        base[1], base[4], base[6], base[9] = -1, p_ring + 2, -(2 ** 40), \
            2 ** 62
        pos[:t_ring] = t.arange(t_ring)  # every row at least once
        pos[t_ring : t_ring + 6] = t.tensor(
            [-1, -t_ring, t_ring + 3, -(2 ** 40), 2 ** 62, -(2 ** 62) - 7]
        )
    else:
        left = t.randint(0, 6, (t_ring,), generator=gen)
        terminal = (t.rand(t_ring, generator=gen) < 0.2).float()
    if kind == "exact":
        reward = t.randint(-3, 4, (t_ring,), generator=gen).float()
        gamma = 0.5
    else:
        reward = t.randn(t_ring, generator=gen)
        gamma = 0.99
    return SimpleNamespace(
        planes=planes, base=base, left=left, reward=reward,
        terminal=terminal, pos=pos, gamma=gamma, kind=kind,
    )


@functools.lru_cache(maxsize=None)
def op_reference(h, w, kind, k, n, p_ring=P_RING, t_ring=T_RING,
                 batch=BATCH):
    c = op_inputs(h, w, kind, p_ring, t_ring, batch)
    return loop_reference(c.planes, c.base, c.left, c.reward, c.terminal,
                          c.pos, k, n, c.gamma)


def run_op(ops, case, k, n, channels_last, device="cpu"):
    cols = [getattr(case, name).to(device) for name in
            ("planes", "base", "left", "reward", "terminal", "pos")]
    return ops.framestack_gather_nstep(
        *cols, k, n, case.gamma, channels_last=channels_last
    )


def check_layout(stack, channels_last):
    if channels_last:
        assert stack.is_contiguous(memory_format=t.channels_last)
    else:
        assert stack.is_contiguous()


def check_op(got, want, kind, channels_last):
    """Outputs of the op against the loop: u8 stacks, terminal_n and
    steps exact; reward bit-equal for the exact case, within the bound
    for random fp32 rewards."""
    state, next_state, reward_n, terminal_n, steps = got
    want_s, want_n, want_r, bound, want_t, want_m = want
    for stack, ref in ((state, want_s), (next_state, want_n)):
        assert stack.dtype == t.uint8 and stack.shape == ref.shape
        check_layout(stack, channels_last)
        assert t.equal(stack.cpu(), ref)
    assert reward_n.dtype == t.float32 and terminal_n.dtype == t.float32
    assert steps.dtype == t.int64
    assert reward_n.shape == terminal_n.shape == steps.shape == want_m.shape
    assert t.equal(steps.cpu(), want_m)
    assert t.equal(terminal_n.cpu(), want_t)
    err = (reward_n.cpu().double() - want_r).abs()
    print(f"{kind}: max reward error {float(err.max()):.3e}, "
          f"smallest bound {float(bound.min()):.3e}")
    if kind == "exact":
        assert t.equal(reward_n.cpu().double(), want_r)
    else:
        assert bool((err <= bound).all())


# -- buffer oracle: the host fold ----------------------------------------
ATTRS = ["state", "action", "reward", "next_state", "terminal", "*"]


def make_episodes(lengths, k=K, h=H, w=W, seed=0):
    """Raw 1-step sliding-window episodes. Rewards are small integers
    (exact n-step sums with gamma 0.5), every transition carries its id
    as the custom attribute ``tid``, and episodes of six or more steps
    also have a terminal at their third step."""
    gen = t.Generator().manual_seed(seed)
    episodes, tid = [], 0
    for length in lengths:
        planes = t.randint(0, 256, (length + k, h, w), dtype=t.uint8,
                           generator=gen)
        episode = []
        for i in range(length):
            episode.append({
                "state": {"state": planes[i : i + k].clone().unsqueeze(0)},
                "action": {"action": t.randint(0, 3, (1, 1),
                                               generator=gen)},
                "next_state": {
                    "state": planes[i + 1 : i + k + 1].clone().unsqueeze(0)
                },
                "reward": float(t.randint(-3, 4, (1,), generator=gen)),
                "terminal": i == length - 1 or (length >= 6 and i == 2),
                "tid": float(tid),
            })
            tid += 1
        episodes.append(episode)
    return episodes


def host_fold(episodes, n, gamma):
    """What RAINBOW stores today: the episodes go through the host fold
    of ``RAINBOW.store_episode`` into a flat ``DeviceTransitionBuffer``
    on the CPU. Returns its columns ordered by ``tid`` plus the length
    ``m`` of every transition's window."""
    from machin_amd.frame.algorithms import RAINBOW
    from machin_amd.frame.buffers import DeviceTransitionBuffer

    total = sum(len(e) for e in episodes)
    flat = DeviceTransitionBuffer(total, "cpu")
    algo = SimpleNamespace(
        reward_future_steps=n, discount=gamma, replay_buffer=flat
    )
    for episode in episodes:
        RAINBOW.store_episode(algo, episode)
    assert flat.size() == total
    data = flat._inner.data
    order = data["tid"].long().argsort()
    assert t.equal(data["tid"][order].long(), t.arange(total))
    rows = {key: col[order] for key, col in data.items()}
    rows["m"] = t.tensor(
        [min(n, len(e) - i) for e in episodes for i in range(len(e))]
    )
    return rows


@functools.lru_cache(maxsize=None)
def round_trip_oracle(stores, n, gamma):
    episodes = make_episodes([LENGTHS[i % len(LENGTHS)]
                              for i in range(stores)])
    return episodes, host_fold(episodes, n, gamma)


class NStepRingModel:
    """Which ids are live, from first principles: every plane write
    stamps its slot; a transition is live while all m+k slots of its
    window still carry the stamps it was written with."""

    def __init__(self, frames, n, k=K):
        self.frames, self.n, self.k = frames, n, k
        self.stamp = [None] * frames
        self.head = 0
        self.clock = 0
        self.windows = {}

    def store(self, ids):
        slots = []
        for _ in range(len(ids) + self.k):
            self.stamp[self.head] = self.clock
            slots.append((self.head, self.clock))
            self.head = (self.head + 1) % self.frames
            self.clock += 1
        for i, tid in enumerate(ids):
            m = min(self.n, len(ids) - i)
            self.windows[tid] = slots[i : i + m + self.k]
            assert len(self.windows[tid]) == m + self.k

    def live(self):
        return {
            tid for tid, win in self.windows.items()
            if all(self.stamp[s] == c for s, c in win)
        }


def check_rows(batch, rows, live):
    """Every sampled row equals the host-fold row of a live id."""
    state, action, reward, next_state, terminal, others = batch
    assert set(others) == {"tid", "n_step"}
    ids = others["tid"].view(-1).cpu().long()
    assert set(ids.tolist()) <= live
    assert t.equal(state["state"].cpu(), rows["state/state"][ids])
    assert t.equal(next_state["state"].cpu(),
                   rows["next_state/state"][ids])
    assert t.equal(action["action"].cpu(), rows["action/action"][ids])
    assert reward.shape == terminal.shape == (len(ids), 1)
    assert reward.dtype == terminal.dtype == t.float32
    assert t.equal(reward.view(-1).cpu(), rows["reward"][ids])
    assert t.equal(terminal.view(-1).cpu(), rows["terminal"][ids])
    steps = others["n_step"]
    assert steps.dtype == t.int64 and steps.shape == (len(ids), 1)
    assert t.equal(steps.view(-1).cpu(), rows["m"][ids])
    return set(ids.tolist())


def round_trip(device, stores=32, frames=40, draws=2000, n=3, gamma=0.5,
               **kwargs):
    """Wrap/eviction round trip with n-step sampling: after every store
    the buffer's size and its samples agree with the liveness model and
    the host fold."""
    from machin_amd.frame.buffers import DeviceFrameStackBuffer

    episodes, rows = round_trip_oracle(stores, n, gamma)
    buf = DeviceFrameStackBuffer(frames, device, n_step=n, discount=gamma,
                                 **kwargs)
    model = NStepRingModel(frames, n)
    batch = None
    for episode in episodes:
        buf.store_episode(episode)
        model.store([int(tr["tid"]) for tr in episode])
        live = model.live()
        assert buf.size() == len(buf) == len(live)
        n_drawn, batch = buf.sample_batch(draws, sample_attrs=ATTRS)[:2]
        assert n_drawn == draws
        # miss probability per id <= (35/36)^2000
        assert check_rows(batch, rows, live) == live
    return buf, batch
