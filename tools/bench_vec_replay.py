"""Time the hop from the device env to the frame-deduplicated replay.

    python tools/bench_vec_replay.py [--out table.md] [--json]

Two ways of getting one vector step of ``DevicePixelCatchVecEnv`` (the
default env: 5 balls, 135-step episodes) into a prioritized ``n_step=3``
replay are timed, for E in {256, 4096} envs:

* episodes — ``env.step`` with ``record=True``, ``finished_episodes()``
             (one read of ``[E]`` lengths, a wait for the device) and
             one ``DeviceFrameStackBuffer.store_frames`` per episode;
* per-step — ``env.step`` with ``record=False`` and one
             ``DeviceVecFrameStackBuffer.append_step``.

Method: the episode path waits for the device, so both are timed by the
wall clock over a window of whole vector steps with a device
synchronize at both ends. All envs are reset together and every episode
is 135 steps, so the episodes of all envs end on the same vector step;
a window is therefore a multiple of 135 steps and holds one episode per
env and 135 steps — the average a desynchronised run has per step (E /
135 episodes). Each path is warmed up over one window; then ``--rounds``
rounds alternate the two paths in one process; the median round is
reported with the min-max spread. Both replays hold ``E * 256`` frames.

The append kernel alone (``ops.framestack_vec_append`` on the per-step
buffer's rings, 1 lane in 135 ended) is timed with device events. Its
bytes are ``E * 7056`` read and ``E * 7056`` written, plus the mirror
copy for the (k + n) / S of the lanes whose slot has one and ``2 * 4 *
7056`` per ended lane, set against the ~6.3 TB/s that streaming kernels
reach on an MI355X. Needs a GPU; there is no CPU mode.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch as t

from machin_amd import ops
from machin_amd.env.envs import DevicePixelCatchVecEnv
from machin_amd.frame.buffers import (
    DeviceFrameStackBuffer, DeviceVecFrameStackBuffer,
)

PLANE = 84 * 84
STREAM_GBPS = 6300.0
EPISODE = 135
LANE_SLOTS = 256
K, N_STEP = 4, 3


class EpisodePath:
    name = "episodes"

    def __init__(self, E, dev):
        self.env = DevicePixelCatchVecEnv(E, dev, seed=1, record=True)
        self.buffer = DeviceFrameStackBuffer(
            E * LANE_SLOTS, dev, frame_stack=K, prioritized=True,
            n_step=N_STEP,
        )
        self.env.reset()

    def step(self, action):
        self.env.step(action)
        for frames, cols in self.env.finished_episodes():
            self.buffer.store_frames(frames, {
                "action/action": cols["action"],
                "reward": cols["reward"],
                "terminal": cols["terminal"],
            })


class StepPath:
    name = "per_step"

    def __init__(self, E, dev):
        self.env = DevicePixelCatchVecEnv(E, dev, seed=1, record=False)
        self.buffer = DeviceVecFrameStackBuffer(
            E, LANE_SLOTS, dev, frame_stack=K, prioritized=True,
            n_step=N_STEP,
        )
        self.buffer.begin(self.env.reset())

    def step(self, action):
        obs, reward, done, info = self.env.step(action)
        self.buffer.append_step(action, reward, done, info["frame"], obs)


def window_ms(path, draws, steps):
    """Wall-clock ms per vector step over ``steps`` steps."""
    t.cuda.synchronize()
    start = time.perf_counter()
    for i in range(steps):
        path.step(draws[i % len(draws)])
    t.cuda.synchronize()
    return (time.perf_counter() - start) * 1e3 / steps


def kernel_ms(path, iters):
    """Device-event ms of one framestack_vec_append on the path's own
    rings and the env's resident tensors; 1 lane in 135 ends."""
    buf, env = path.buffer, path.env
    E = buf.num_lanes
    done = (t.rand(E, device=buf.buffer_device) < 1.0 / EPISODE).float()
    args = (buf._planes, buf._reward, buf._terminal, buf._left, buf._head,
            buf._run, env._frame, env._obs, env._reward, done, done,
            buf._one, K, N_STEP)
    for _ in range(5):
        ops.framestack_vec_append(*args)
    start = t.cuda.Event(enable_timing=True)
    stop = t.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        ops.framestack_vec_append(*args)
    stop.record()
    stop.synchronize()
    ended = int(done.sum())
    nbytes = PLANE * (E * (2 + (K + N_STEP) / LANE_SLOTS) + ended * 2 * K)
    return start.elapsed_time(stop) / iters, nbytes, ended


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--rounds", type=int, default=7)
    parser.add_argument("--windows", type=int, default=1,
                        help="episodes (135 steps) per timed window")
    parser.add_argument("--out", default=None)
    parser.add_argument("--json", action="store_true",
                        help="write the raw rows to "
                             "profiles/vec_replay_bench.json")
    args = parser.parse_args()
    if not t.cuda.is_available():
        raise SystemExit("bench_vec_replay needs a GPU")
    dev = t.device("cuda:0")
    t.manual_seed(0)
    steps = EPISODE * args.windows

    rows = []
    for E in (256, 4096):
        paths = [EpisodePath(E, dev), StepPath(E, dev)]
        draws = [t.randint(0, 3, (E,), device=dev) for _ in range(16)]
        for path in paths:
            window_ms(path, draws, EPISODE)  # warm-up, one episode each
        samples = {path.name: [] for path in paths}
        for _ in range(args.rounds):
            for path in paths:
                samples[path.name].append(window_ms(path, draws, steps))
        row = {"E": E, "steps_per_window": steps, "rounds": args.rounds}
        for name, vals in samples.items():
            row[name + "_ms"] = statistics.median(vals)
            row[name + "_min_ms"] = min(vals)
            row[name + "_max_ms"] = max(vals)
        spread = max(row["episodes_max_ms"] - row["episodes_min_ms"],
                     row["per_step_max_ms"] - row["per_step_min_ms"])
        row["spread_ms"] = spread
        row["faster_beyond_spread"] = \
            row["episodes_ms"] - row["per_step_ms"] > spread
        tree_depth = paths[1].buffer._tree.depth
        row["per_step_launches"] = 1 + 1 + tree_depth + 1
        ms, nbytes, ended = kernel_ms(paths[1], 200)
        row["append_kernel_ms"] = ms
        row["append_kernel_bytes"] = nbytes
        row["append_kernel_ended_lanes"] = ended
        row["append_kernel_GBps"] = nbytes / (ms * 1e-3) / 1e9
        rows.append(row)
        print(json.dumps(row), flush=True)
        del paths
        t.cuda.empty_cache()

    lines = [
        "| E | episodes: ms / vector step (min-max) | per-step: ms / vector "
        "step (min-max) | episodes / per-step | beyond the spread | "
        "per-step launches | append kernel ms | append kernel GB/s "
        "(of 6300) |",
        "|---|---|---|---|---|---|---|---|",
    ]
    for r in rows:
        lines.append(
            f"| {r['E']} | {r['episodes_ms']:.3f} "
            f"({r['episodes_min_ms']:.3f}-{r['episodes_max_ms']:.3f}) | "
            f"{r['per_step_ms']:.3f} "
            f"({r['per_step_min_ms']:.3f}-{r['per_step_max_ms']:.3f}) | "
            f"{r['episodes_ms'] / r['per_step_ms']:.1f}x | "
            f"{'yes' if r['faster_beyond_spread'] else 'NO'} | "
            f"{r['per_step_launches']} | {r['append_kernel_ms']:.4f} | "
            f"{r['append_kernel_GBps']:.0f} "
            f"({100 * r['append_kernel_GBps'] / STREAM_GBPS:.0f} %) |"
        )
    table = "\n".join(lines)
    print(table)
    if args.out:
        with open(args.out, "w") as f:
            f.write(table + "\n")
    if args.json:
        with open(os.path.join(ROOT, "profiles", "vec_replay_bench.json"),
                  "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
