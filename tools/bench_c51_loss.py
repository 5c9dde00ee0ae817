"""Time RAINBOW's C51 loss head: the eager chain against the fused op.

    python tools/bench_c51_loss.py [--out table.md] [--json rows.json]

For A=6 actions, N=51 atoms, B in {32, 512, 4096}, fp32 and bf16
inputs, the step from the three network outputs ``[B, A, N]`` to the
per-sample loss AND the gradient with respect to the online net's
output (forward plus backward with a given ``g [B]``) is timed on the
GPU in these forms:

* eager         — the chain of ``RAINBOW.update`` without
                  ``fused_loss`` (linspace, mul, sum, argmax, two
                  gathers, ``ops.categorical_projection``, clamp, log,
                  mul, sum), on probabilities;
* eager+softmax — the same chain fed by three softmaxes of logits (what
                  a probability-returning model adds to the step; the
                  fair partner of the logits kernel);
* fallback      — ``ops._c51_loss_torch`` on the device, probabilities;
* kernel        — ``ops.c51_loss`` (one gfx950 kernel each way),
                  probabilities;
* kernel logits — ``ops.c51_loss(from_logits=True)`` on the logits.

Method: the forms are first checked to agree (``rtol=1e-4,
atol=1e-3``); then each is warmed up and timed with device events over
``--iters`` calls, ``--rounds`` times, alternating the forms inside a
round so that clocks and load are shared; the median round is reported
with the min-max spread. Needs a GPU; there is no CPU mode.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(
    0, os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
)

import torch as t

from machin_amd import ops

A, N = 6, 51
V_MIN, V_MAX = -10.0, 10.0
GAMMA_N = 0.99 ** 3


def eager_chain(dist, action, next_online, next_target, reward, terminal):
    B = dist.shape[0]
    device = dist.device
    with t.no_grad():
        support = t.linspace(V_MIN, V_MAX, N, device=device)
        next_q = (next_online * support.view(1, 1, N)).sum(dim=2)
        best = next_q.argmax(dim=1)
        next_dist = next_target[t.arange(B, device=device), best]
        reward = reward.to(device).float().view(B)
        terminal = terminal.to(device).float().view(B)
        proj = ops.categorical_projection(
            next_dist, reward, terminal, GAMMA_N, V_MIN, V_MAX
        )
    pred = dist[t.arange(B, device=device), action]
    log_pred = t.log(pred.clamp_min(1e-8))
    return -(proj * log_pred).sum(dim=1)


def make_inputs(B, dtype, dev):
    gen = t.Generator(device="cpu").manual_seed(B)
    logits = [t.randn(B, A, N, generator=gen) for _ in range(3)]
    z = t.linspace(V_MIN, V_MAX, N)
    star = t.randint(0, A, (B,), generator=gen)
    logits[1][t.arange(B), star] += 2.0 * z / V_MAX
    logits = [x.to(dtype).to(dev) for x in logits]
    probs = [t.softmax(x.float(), dim=-1).to(dtype) for x in logits]
    rest = (
        t.randint(0, A, (B,), generator=gen).to(dev),
        (4.0 * t.randn(B, generator=gen)).to(dev),
        (t.rand(B, generator=gen) > 0.8).float().to(dev),
    )
    g = t.randn(B, generator=gen).to(dev)
    return logits, probs, rest, g


def time_ms(fn, iters):
    start = t.cuda.Event(enable_timing=True)
    stop = t.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--iters", type=int, default=300)
    parser.add_argument("--rounds", type=int, default=7)
    parser.add_argument("--out", default=None, help="markdown table")
    parser.add_argument("--json", default=None, help="raw rows")
    args = parser.parse_args()
    if not t.cuda.is_available():
        raise SystemExit("bench_c51_loss needs a GPU")
    dev = t.device("cuda:0")

    rows = []
    for dtype in (t.float32, t.bfloat16):
        for B in (32, 512, 4096):
            logits, probs, (action, reward, terminal), g = make_inputs(
                B, dtype, dev
            )
            p_dist = probs[0].clone().requires_grad_(True)
            l_dist = logits[0].clone().requires_grad_(True)

            def step(loss_fn, leaf):
                def run():
                    return t.autograd.grad(loss_fn(), leaf, g)[0]
                return run

            def eager():
                return eager_chain(p_dist, action, probs[1], probs[2],
                                   reward, terminal)

            def eager_softmax():
                d = t.softmax(l_dist, dim=-1)
                with t.no_grad():
                    o = t.softmax(logits[1], dim=-1)
                    tg = t.softmax(logits[2], dim=-1)
                return eager_chain(d, action, o, tg, reward, terminal)

            def fallback():
                return ops._c51_loss_torch(
                    p_dist, action, probs[1], probs[2], reward, terminal,
                    GAMMA_N, V_MIN, V_MAX,
                )[0]

            def kernel():
                return ops.c51_loss(
                    p_dist, action, probs[1], probs[2], reward, terminal,
                    GAMMA_N, V_MIN, V_MAX,
                )[0]

            def kernel_logits():
                return ops.c51_loss(
                    l_dist, action, logits[1], logits[2], reward, terminal,
                    GAMMA_N, V_MIN, V_MAX, from_logits=True,
                )[0]

            variants = [
                ("eager", step(eager, p_dist)),
                ("eager_softmax", step(eager_softmax, l_dist)),
                ("fallback", step(fallback, p_dist)),
                ("kernel", step(kernel, p_dist)),
                ("kernel_logits", step(kernel_logits, l_dist)),
            ]
            # same results first; fp32 inputs only (the eager chain
            # rounds its intermediates to bf16, the op computes in fp32)
            if dtype == t.float32:
                for a, b in ((eager, kernel), (fallback, kernel),
                             (eager_softmax, kernel_logits)):
                    assert t.allclose(a(), b(), rtol=1e-4, atol=1e-3)
                want = variants[0][1]()
                assert t.allclose(variants[3][1](), want, rtol=1e-4,
                                  atol=1e-3)
            for _, fn in variants:
                time_ms(fn, 20)  # warm-up
            samples = {name: [] for name, _ in variants}
            for _ in range(args.rounds):
                for name, fn in variants:
                    samples[name].append(time_ms(fn, args.iters))
            row = {"dtype": str(dtype).split(".")[1], "B": B, "A": A,
                   "N": N, "iters": args.iters, "rounds": args.rounds}
            for name, vals in samples.items():
                row[name + "_ms"] = statistics.median(vals)
                row[name + "_min_ms"] = min(vals)
                row[name + "_max_ms"] = max(vals)
            row["eager_over_kernel"] = row["eager_ms"] / row["kernel_ms"]
            row["eager_softmax_over_kernel_logits"] = (
                row["eager_softmax_ms"] / row["kernel_logits_ms"]
            )
            rows.append(row)
            print(json.dumps(row), flush=True)

    def cell(r, name):
        return (f"{r[name + '_ms']:.4f} ({r[name + '_min_ms']:.4f}-"
                f"{r[name + '_max_ms']:.4f})")

    lines = [
        "| dtype | B | eager ms (min-max) | eager+softmax ms | "
        "fallback ms | kernel ms | kernel logits ms | eager / kernel | "
        "eager+softmax / kernel logits |",
        "|---|---|---|---|---|---|---|---|---|",
    ]
    for r in rows:
        lines.append(
            f"| {r['dtype']} | {r['B']} | {cell(r, 'eager')} | "
            f"{cell(r, 'eager_softmax')} | {cell(r, 'fallback')} | "
            f"{cell(r, 'kernel')} | {cell(r, 'kernel_logits')} | "
            f"{r['eager_over_kernel']:.2f}x | "
            f"{r['eager_softmax_over_kernel_logits']:.2f}x |"
        )
    table = "\n".join(lines)
    print(table)
    if args.out:
        with open(args.out, "w") as f:
            f.write(table + "\n")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
