"""Shared helpers for the frame-stack replay tests: sliding-window
episode builder, a plain-python liveness model of the plane ring, and
the wrap/eviction round trip run on CPU and on the GPU."""
import torch as t

K, H, W = 4, 4, 8
LENGTHS = [5, 7, 1, 9, 3, 12, 2, 36, 4, 8, 6, 11, 1, 20, 5, 13]


class Episodes:
    """Builds sliding-window episodes; every transition's reward is a
    unique integer id, and the originals are kept by id."""

    def __init__(self, k=K, h=H, w=W, seed=0):
        self.k, self.h, self.w = k, h, w
        self.gen = t.Generator().manual_seed(seed)
        self.state, self.next_state = [], []
        self.action, self.terminal = [], []

    def make(self, length):
        k = self.k
        planes = t.randint(
            0, 256, (length + k, self.h, self.w), dtype=t.uint8,
            generator=self.gen,
        )
        episode, ids = [], []
        for i in range(length):
            tid = len(self.state)
            st = planes[i : i + k].clone()
            nx = planes[i + 1 : i + k + 1].clone()
            act = int(t.randint(0, 3, (1,), generator=self.gen))
            self.state.append(st)
            self.next_state.append(nx)
            self.action.append(act)
            self.terminal.append(float(i == length - 1))
            ids.append(tid)
            episode.append({
                "state": {"state": st.unsqueeze(0)},
                "action": {"action": t.tensor([[act]])},
                "next_state": {"state": nx.unsqueeze(0)},
                "reward": float(tid),
                "terminal": i == length - 1,
            })
        return episode, ids


class RingModel:
    """Which ids are live, from first principles: every plane write
    stamps its slot; a transition is live while all k+1 slots of its
    window still carry the stamps it was written with."""

    def __init__(self, frames, k=K):
        self.frames, self.k = frames, k
        self.stamp = [None] * frames
        self.head = 0
        self.clock = 0
        self.windows = {}  # id -> [(slot, stamp)] * (k+1)

    def store(self, ids):
        slots = []
        for _ in range(len(ids) + self.k):
            self.stamp[self.head] = self.clock
            slots.append((self.head, self.clock))
            self.head = (self.head + 1) % self.frames
            self.clock += 1
        for i, tid in enumerate(ids):
            self.windows[tid] = slots[i : i + self.k + 1]

    def live(self):
        return {
            tid for tid, win in self.windows.items()
            if all(self.stamp[s] == c for s, c in win)
        }


def check_samples(eps, batch, live):
    """Every sampled row equals the original of a live id."""
    state, action, reward, next_state, terminal = batch
    ids = reward.view(-1).cpu().long()
    assert set(ids.tolist()) <= live
    want_s = t.stack([eps.state[i] for i in ids.tolist()])
    want_n = t.stack([eps.next_state[i] for i in ids.tolist()])
    assert t.equal(state["state"].cpu(), want_s)
    assert t.equal(next_state["state"].cpu(), want_n)
    assert action["action"].view(-1).cpu().tolist() == [
        eps.action[i] for i in ids.tolist()
    ]
    assert terminal.view(-1).cpu().tolist() == [
        eps.terminal[i] for i in ids.tolist()
    ]
    return set(ids.tolist())


ATTRS = ["state", "action", "reward", "next_state", "terminal"]


def round_trip(device, stores=32, frames=40, draws=2000, **kwargs):
    """Wrap/eviction round trip: after every store the buffer's size
    and its samples agree with the liveness model."""
    from machin_amd.frame.buffers import DeviceFrameStackBuffer

    buf = DeviceFrameStackBuffer(frames, device, **kwargs)
    eps, model = Episodes(), RingModel(frames)
    for i in range(stores):
        episode, ids = eps.make(LENGTHS[i % len(LENGTHS)])
        buf.store_episode(episode)
        model.store(ids)
        live = model.live()
        assert buf.size() == len(buf) == len(live)
        n, batch = buf.sample_batch(draws, sample_attrs=ATTRS)
        assert n == draws
        # miss probability per id <= (35/36)^2000
        assert check_samples(eps, batch, live) == live
    return buf, batch
