"""Shared by test_framestack_vec_cpu / _gpu: a plain Python model (the
LEDGER) of what a ``DeviceVecFrameStackBuffer`` must hold after any
sequence of ``begin`` / ``append_step`` calls, scripted step streams,
and the comparisons against it.

The ledger never looks at the op: per lane it keeps the episodes as
lists of planes, rewards and terminals plus the number of planes
written, and derives the set of sampleable transitions (window
complete, base plane not overwritten) and the tuple each of them must
gather to. Rewards are drawn from {-1, 0, 1} and the discount is 0.5,
so every float32 fold is exact in any order and every comparison is
``torch.equal``.
"""
from contextlib import contextmanager

import numpy as np
import torch as t

from machin_amd import ops
from machin_amd.frame.buffers import DeviceVecFrameStackBuffer

DISCOUNT = 0.5
FRAMES = [(4, 8), (5, 7)]
ENDS = ["never", "always", "p15", "p60", "in_mirror", "last_slot"]


class Ledger:
    def __init__(self, E, S, k, n, discount=DISCOUNT):
        self.E, self.S, self.k, self.n = E, S, k, n
        self.R = S + k + n
        self.discount = discount
        self.head = [0] * E
        # per lane: episodes, each {"start", "planes", "reward",
        # "terminal", "ended"}; the last one is the running episode
        self.lanes = [[] for _ in range(E)]

    def _open(self, e, planes):
        self.lanes[e].append({
            "start": self.head[e], "planes": [p.copy() for p in planes],
            "reward": [], "terminal": [], "ended": False,
        })
        self.head[e] += self.k

    def begin(self, obs):
        """obs: u8 array [E, k, H, W]. Running episodes stay as they
        are, un-ended: only their complete windows count."""
        for e in range(self.E):
            self._open(e, obs[e])

    def step(self, frame, first, reward, terminal, done):
        for e in range(self.E):
            ep = self.lanes[e][-1]
            ep["planes"].append(frame[e].copy())
            ep["reward"].append(float(reward[e]))
            ep["terminal"].append(float(terminal[e]))
            self.head[e] += 1
            if done[e] != 0:
                ep["ended"] = True
                self._open(e, first[e])
            # forget episodes whose every plane is overwritten
            self.lanes[e] = [
                p for p in self.lanes[e]
                if p["start"] + len(p["planes"]) + self.S > self.head[e]
            ]

    def expected(self):
        """{flat position: (state, next_state, reward_n, terminal_n, m)}
        of every sampleable transition."""
        k, n, S, out = self.k, self.n, self.S, {}
        for e in range(self.E):
            for ep in self.lanes[e]:
                L = len(ep["reward"])
                for i in range(L):
                    if ep["ended"]:
                        m = min(n, L - i)
                    elif i + n <= L:
                        m = n
                    else:
                        continue  # window not complete
                    base = ep["start"] + i
                    if self.head[e] > base + S:
                        continue  # base plane overwritten
                    acc, disc, term = 0.0, 1.0, 0.0
                    for j in range(m):
                        acc += disc * ep["reward"][i + j]
                        term = max(term, ep["terminal"][i + j])
                        disc *= self.discount * (1.0 - ep["terminal"][i + j])
                    pos = e * self.R + base % S
                    assert pos not in out
                    out[pos] = (
                        np.stack(ep["planes"][i:i + k]),
                        np.stack(ep["planes"][i + m:i + m + k]),
                        acc, term, m,
                    )
        return out


def done_script(kind, E, S, G, seed):
    """done(step, heads) -> f32 array [E]; heads are the lanes' plane
    counts before the step."""
    rng = np.random.RandomState(seed + 17)

    def done(step, heads):
        i = np.asarray(heads) % S
        if kind == "never":
            d = np.zeros(E, bool)
        elif kind == "always":
            d = np.ones(E, bool)
        elif kind in ("p15", "p60"):
            d = rng.rand(E) < (0.15 if kind == "p15" else 0.6)
        elif kind == "in_mirror":
            # ends with head mod S inside the mirrored slots
            d = (i < G) & ((step + np.arange(E)) % 2 == 0)
        elif kind == "last_slot":
            d = i == S - 1
        else:
            raise ValueError(kind)
        return d.astype(np.float32)

    return done


def stream(E, H, W, k, S, steps, kind, G, seed=0, time_limit=False):
    """Yield the inputs of a scripted run: first ("begin", obs), then
    ("step", action, reward, done, frame, first, terminal) per step,
    all numpy. ``time_limit``: every other episode end has terminal 0."""
    rng = np.random.RandomState(seed)
    done_fn = done_script(kind, E, S, G, seed)
    heads = np.full(E, k)
    yield ("begin", rng.randint(0, 256, (E, k, H, W)).astype(np.uint8))
    ends = 0
    for step in range(steps):
        done = done_fn(step, heads)
        terminal = done.copy()
        if time_limit:
            for e in range(E):
                if done[e]:
                    ends += 1
                    if ends % 2 == 0:
                        terminal[e] = 0.0
        yield (
            "step",
            rng.randint(0, 3, (E, 1)).astype(np.int64),
            rng.randint(-1, 2, E).astype(np.float32),
            done,
            rng.randint(0, 256, (E, H, W)).astype(np.uint8),
            rng.randint(0, 256, (E, k, H, W)).astype(np.uint8),
            terminal,
        )
        heads = heads + 1 + k * (done != 0)


def make_buffer(E, S, k, n, device, **kwargs):
    kwargs.setdefault("discount", DISCOUNT)
    return DeviceVecFrameStackBuffer(
        E, S, device, frame_stack=k, n_step=n, **kwargs
    )


def to_dev(a, device, channels_last=False):
    x = t.from_numpy(a).to(device)
    if channels_last:
        x = x.contiguous(memory_format=t.channels_last)
    return x


def feed(buf, item, channels_last=False, frame_view=None):
    """Give one item of :func:`stream` to a buffer."""
    dev = buf.buffer_device
    if item[0] == "begin":
        buf.begin(to_dev(item[1], dev, channels_last))
        return
    _, action, reward, done, frame, first, terminal = item
    frame = to_dev(frame, dev)
    if frame_view is not None:
        frame = frame_view(frame)
    buf.append_step(
        to_dev(action, dev), to_dev(reward, dev), to_dev(done, dev), frame,
        to_dev(first, dev, channels_last), to_dev(terminal, dev),
    )


def feed_ledger(ledger, item):
    if item[0] == "begin":
        ledger.begin(item[1])
    else:
        _, _, reward, done, frame, first, terminal = item
        ledger.step(frame, first, reward, terminal, done)


@contextmanager
def append_op(fn, record=None):
    """Route ``ops.framestack_vec_append`` (what ``append_step`` calls)
    to ``fn`` and keep what it returns."""
    orig = ops.framestack_vec_append

    def wrapper(*args):
        out = fn(*args)
        if record is not None:
            record.append(out)
        return out

    ops.framestack_vec_append = wrapper
    try:
        yield
    finally:
        ops.framestack_vec_append = orig


def gather_all(buf, pos):
    """(state, next_state, reward_n, terminal_n, m) of the flat
    positions ``pos`` through the existing gather ops."""
    k, n = buf.frame_stack, buf.n_step
    if n > 1:
        return ops.framestack_gather_nstep(
            buf._planes, buf._base, buf._left, buf._reward, buf._terminal,
            pos, k, n, buf.discount,
        )
    state, next_state = ops.framestack_gather(buf._planes, pos, k)
    return (
        state, next_state, buf._reward.index_select(0, pos),
        buf._terminal.index_select(0, pos), t.ones_like(pos),
    )


def check_ledger(buf, ledger):
    """The positive leaves are exactly the ledger's set and gather the
    ledger's tuples; mirror leaves are 0."""
    want = ledger.expected()
    leaves = buf._tree.get_leaf_all_weights()
    pos = (leaves > 0).nonzero().view(-1)
    assert pos.tolist() == sorted(want), (
        f"sampleable positions {pos.tolist()} != ledger {sorted(want)}"
    )
    if not want:
        return 0
    state, next_state, reward, terminal, m = gather_all(buf, pos)
    rows = [want[p] for p in sorted(want)]
    dev = buf.buffer_device
    assert t.equal(state, to_dev(np.stack([r[0] for r in rows]), dev))
    assert t.equal(next_state, to_dev(np.stack([r[1] for r in rows]), dev))
    assert t.equal(reward, t.tensor([r[2] for r in rows],
                                    dtype=t.float32, device=dev))
    assert t.equal(terminal, t.tensor([r[3] for r in rows],
                                      dtype=t.float32, device=dev))
    assert t.equal(m, t.tensor([r[4] for r in rows], dtype=t.int64,
                               device=dev))
    return len(want)


def ring_state(buf):
    """Everything a step may change, by name."""
    return {
        "planes": buf._planes, "reward": buf._reward,
        "terminal": buf._terminal, "left": buf._left, "head": buf._head,
        "run": buf._run, "action": buf._action,
        "tree": buf._tree.weights,
    }


def all_transitions(planes, base, left, reward, terminal, action, pos, k, n,
                    discount):
    """Sorted list of (state bytes, next_state bytes, action, reward_n,
    terminal_n, m) of the positions ``pos`` of a flat ring."""
    state, next_state, r, d, m = ops.framestack_gather_nstep(
        planes, base, left, reward, terminal, pos, k, n, discount
    )
    act = action.index_select(0, pos).view(-1)
    return sorted(
        (state[i].cpu().numpy().tobytes(),
         next_state[i].cpu().numpy().tobytes(),
         int(act[i]), float(r[i]), float(d[i]), int(m[i]))
        for i in range(pos.numel())
    )


def env_against_episode_path(device, layout="nchw"):
    """The same 54 vector steps of a 3-env PixelCatch (balls=1: every
    episode is 27 steps) go to a DeviceVecFrameStackBuffer through
    append_step and to a DeviceFrameStackBuffer through
    finished_episodes / store_frames; returns both sorted transition
    lists."""
    from machin_amd.env.envs import DevicePixelCatchVecEnv
    from machin_amd.frame.buffers import DeviceFrameStackBuffer

    k, n = 4, 3
    env = DevicePixelCatchVecEnv(3, device, balls=1, record=True,
                                 layout=layout)
    vec = make_buffer(3, 80, k, n, device, prioritized=True)
    ref = DeviceFrameStackBuffer(
        600, device, frame_stack=k, prioritized=True, n_step=n,
        discount=DISCOUNT,
    )
    gen = t.Generator().manual_seed(3)
    obs = env.reset()
    vec.begin(obs)
    for _ in range(54):
        action = t.randint(0, 3, (3,), generator=gen).to(device)
        obs, reward, done, info = env.step(action)
        vec.append_step(action, reward, done, info["frame"], obs)
        for frames, cols in env.finished_episodes():
            ref.store_frames(frames, {
                "action/action": cols["action"],
                "reward": cols["reward"],
                "terminal": cols["terminal"],
            })
    pos = (vec._tree.get_leaf_all_weights() > 0).nonzero().view(-1)
    got = all_transitions(
        vec._planes, vec._base, vec._left, vec._reward, vec._terminal,
        vec._action, pos, k, n, DISCOUNT,
    )
    data = ref._inner.data
    assert ref.size() == ref._t_count  # nothing evicted
    want = all_transitions(
        ref._planes, data["_base"], data["_left"], data["reward"],
        data["terminal"], data["action/action"],
        t.arange(ref.size(), device=device), k, n, DISCOUNT,
    )
    return got, want, vec
