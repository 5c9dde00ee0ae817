"""Time the device-resident batched PixelCatch env.

    python tools/bench_device_env.py [--out table.md]

For E in {256, 4096, 32768} envs, in both observation layouts, with the
episode recorder off (and on at E = 4096), three ways of stepping
PixelCatch are timed:

* kernel   — ``ops.pixelcatch_step`` (one gfx950 kernel per call);
* fallback — the same step as a torch composition on the SAME device
             tensors (``ops._pixelcatch_step_torch``);
* host     — ``PixelCatchEnv`` on one CPU core, wall clock over at
             least ``--host-seconds`` (per env-step, independent of E).

Method (as tools/bench_framestack.py): kernel and fallback are first
checked to produce the same bytes over ``--check-steps`` calls from the
same reset; then each is warmed up and timed with device events over a
number of calls, ``--rounds`` times, alternating the variants inside a
round; the median round is reported with the min-max spread. Actions
are fresh random draws per call. The bytes a call must write are
``E * (4 + 1) * 7056`` (the stack and the newest plane; ``+ 7056`` per
env with the recorder, more on an episode's first step, which is not
counted) and are set against the ~6.3 TB/s that streaming kernels
reach on an MI355X. Needs a GPU; there is no CPU mode.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(
    0, os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
)

import torch as t

from machin_amd import ops
from machin_amd.env.envs import DevicePixelCatchVecEnv, PixelCatchEnv

PLANE = 84 * 84
STREAM_TBPS = 6.3


def step_with(fn, env, action):
    fn(env._state, env._ball_no, action, env._obs, env._frame, env._reward,
       env._done, env._ep_len, env._seed, env.balls, env.max_episode_steps,
       env.auto_reset, env._log)


def time_ms(fn, env, draws, iters):
    start = t.cuda.Event(enable_timing=True)
    stop = t.cuda.Event(enable_timing=True)
    start.record()
    for i in range(iters):
        step_with(fn, env, draws[i % len(draws)])
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def host_rate(seconds):
    env = PixelCatchEnv(seed=0)
    env.reset()
    steps, start = 0, time.perf_counter()
    while True:
        for _ in range(256):
            _, _, done, _ = env.step(steps % 3)
            steps += 1
            if done:
                env.reset()
        elapsed = time.perf_counter() - start
        if elapsed >= seconds:
            return steps / elapsed


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--rounds", type=int, default=7)
    parser.add_argument("--check-steps", type=int, default=40)
    parser.add_argument("--host-seconds", type=float, default=2.0)
    parser.add_argument("--out", default=None)
    args = parser.parse_args()
    if not t.cuda.is_available():
        raise SystemExit("bench_device_env needs a GPU")
    dev = t.device("cuda:0")
    t.manual_seed(0)

    host = host_rate(args.host_seconds)
    print(json.dumps({"host_env_steps_per_s": host}), flush=True)

    variants = [("kernel", ops.pixelcatch_step),
                ("fallback", ops._pixelcatch_step_torch)]
    cases = [(E, layout, False) for layout in ("nchw", "nhwc")
             for E in (256, 4096, 32768)]
    cases += [(4096, layout, True) for layout in ("nchw", "nhwc")]
    rows = []
    for E, layout, record in cases:
        # short episodes in the check so that resets are compared too
        envs = {
            name: DevicePixelCatchVecEnv(
                E, dev, seed=1, balls=1, max_episode_steps=17,
                layout=layout, record=record)
            for name, _ in variants
        }
        draws = [t.randint(0, 3, (E,), device=dev) for _ in range(16)]
        for env in envs.values():
            env.reset()
        for i in range(args.check_steps):
            for name, fn in variants:
                step_with(fn, envs[name], draws[i % 16])
            a, b = envs["kernel"], envs["fallback"]
            for x, y in ((a._obs, b._obs), (a._frame, b._frame),
                         (a._reward, b._reward), (a._done, b._done),
                         (a._state, b._state), (a._ball_no, b._ball_no)):
                assert t.equal(x, y)
            assert a._obs.stride() == b._obs.stride()
        if record:
            for x, y in zip(envs["kernel"]._log, envs["fallback"]._log):
                assert t.equal(x, y)
        del envs
        # the timed envs have the default episode (5 balls, 135 steps)
        envs = {
            name: DevicePixelCatchVecEnv(E, dev, seed=1, layout=layout,
                                         record=record)
            for name, _ in variants
        }
        for env in envs.values():
            env.reset()
        # timed windows of 40-70 ms (kernel) and 0.2-0.6 s (fallback)
        iters = {"kernel": max(64, min(4000, 2 ** 23 // E)),
                 "fallback": max(8, min(200, 2 ** 19 // E))}
        for name, fn in variants:
            time_ms(fn, envs[name], draws, 5)  # warm-up
        samples = {name: [] for name, _ in variants}
        for _ in range(args.rounds):
            for name, fn in variants:
                samples[name].append(
                    time_ms(fn, envs[name], draws, iters[name]))
        row = {"layout": layout, "E": E, "record": record}
        for name, vals in samples.items():
            row[name + "_ms"] = statistics.median(vals)
            row[name + "_min_ms"] = min(vals)
            row[name + "_max_ms"] = max(vals)
        nbytes = E * (5 + int(record)) * PLANE
        row["kernel_steps_per_s"] = E / (row["kernel_ms"] * 1e-3)
        row["fallback_steps_per_s"] = E / (row["fallback_ms"] * 1e-3)
        row["kernel_GBps"] = nbytes / (row["kernel_ms"] * 1e-3) / 1e9
        row["faster_beyond_spread"] = \
            row["kernel_max_ms"] < row["fallback_min_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del envs
        t.cuda.empty_cache()

    lines = [
        "| layout | E | record | kernel ms (min-max) | fallback on device "
        "ms (min-max) | kernel env-steps/s | fallback env-steps/s | "
        "kernel GB/s written (of 6300) | fallback / kernel | kernel / "
        "one host core |",
        "|---|---|---|---|---|---|---|---|---|---|",
    ]
    for r in rows:
        lines.append(
            f"| {r['layout']} | {r['E']} | {'on' if r['record'] else 'off'}"
            f" | {r['kernel_ms']:.4f} "
            f"({r['kernel_min_ms']:.4f}-{r['kernel_max_ms']:.4f}) | "
            f"{r['fallback_ms']:.3f} "
            f"({r['fallback_min_ms']:.3f}-{r['fallback_max_ms']:.3f}) | "
            f"{r['kernel_steps_per_s'] / 1e6:.1f} M | "
            f"{r['fallback_steps_per_s'] / 1e6:.2f} M | "
            f"{r['kernel_GBps']:.0f} "
            f"({100 * r['kernel_GBps'] / (1e3 * STREAM_TBPS):.0f} %) | "
            f"{r['fallback_ms'] / r['kernel_ms']:.1f}x | "
            f"{r['kernel_steps_per_s'] / host:.0f}x |"
        )
    lines.append("")
    lines.append(
        f"Host `PixelCatchEnv` on one core: {host:.0f} env-steps/s. "
        f"Kernel faster than the fallback beyond the rounds' min-max "
        f"spread in {sum(r['faster_beyond_spread'] for r in rows)} of "
        f"{len(rows)} rows."
    )
    table = "\n".join(lines)
    print(table)
    if args.out:
        with open(args.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
