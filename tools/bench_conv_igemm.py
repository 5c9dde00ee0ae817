"""Time conv2 and conv3 of the Nature CNN, forward and backward apart:
the implicit-GEMM kernels (``impl="hip"``) against the library
composition (``impl="miopen"``).

    python tools/bench_conv_igemm.py [--out table.md] [--json rows.json]
        [--batches 32,512,4096,40960] [--iters 50] [--rounds 5]

For ``ConvBiasReLU2d(32, 64, 4, stride=2)`` on 20x20 inputs and
``ConvBiasReLU2d(64, 64, 3, stride=1, flatten=True)`` on 9x9 inputs,
bf16 parameters and channels-last bf16 ``x``:

* forward  — ``y = conv(x)`` (conv + bias + ReLU);
* backward — gradients of ``x``, weight and bias for a given ``dy`` on
             a graph built once (ReLU mask + bias gradient, data
             gradient, weight gradient; the weight gradient is the
             library's in both forms).

Method: each form runs 10 times first, which also lets the library
finish choosing its algorithms; then it is timed with device events over
``--iters`` calls, ``--rounds`` times, the two forms alternating inside a
round so that clocks and load are shared; the median round is reported
with the min-max spread. The byte floor is the activation traffic of the
direction (forward: x in, y out; backward: dy and y in, g out and read
back once, x in, dx out) at 5.5 TB/s. Needs a GPU; there is no CPU mode."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(
    0, os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
)

import torch as t

from machin_amd.ops.fused_conv import ConvBiasReLU2d

# name, module arguments, input H = W
LAYERS = (
    ("conv2", dict(in_channels=32, out_channels=64, kernel_size=4, stride=2),
     20),
    ("conv3", dict(in_channels=64, out_channels=64, kernel_size=3, stride=1,
                   flatten=True), 9),
)
IMPLS = ("hip", "miopen")
HBM_BYTES_PER_MS = 5.5e9


def time_ms(fn, iters):
    start = t.cuda.Event(enable_timing=True)
    stop = t.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def bench_layer(name, kwargs, hw, batch, args, dev):
    gen = t.Generator().manual_seed(batch + hw)
    cin, cout = kwargs["in_channels"], kwargs["out_channels"]
    ohw = (hw - kwargs["kernel_size"]) // kwargs["stride"] + 1
    x = t.randn(batch, cin, hw, hw, generator=gen).to(dev, t.bfloat16)
    x = x.contiguous(memory_format=t.channels_last).requires_grad_()
    variants = []
    for impl in IMPLS:
        t.manual_seed(0)
        conv = ConvBiasReLU2d(impl=impl, **kwargs).to(dev, t.bfloat16)
        y = conv(x)
        dy = t.randn(y.shape, generator=gen).to(dev, t.bfloat16)
        wrt = [x, conv.weight, conv.bias]
        variants.append((
            impl,
            lambda conv=conv: conv(x),
            lambda y=y, dy=dy, wrt=wrt: t.autograd.grad(
                y, wrt, dy, retain_graph=True),
        ))
    row = {"layer": name, "N": batch, "iters": args.iters,
           "rounds": args.rounds}
    act_in, act_out = 2 * cin * hw * hw, 2 * cout * ohw * ohw
    row["fwd_floor_ms"] = batch * (act_in + act_out) / HBM_BYTES_PER_MS
    row["bwd_floor_ms"] = batch * (4 * act_out + 2 * act_in) / HBM_BYTES_PER_MS
    for which, index in (("fwd", 1), ("bwd", 2)):
        for v in variants:
            time_ms(v[index], 10)  # warm-up, algorithm search
        samples = {v[0]: [] for v in variants}
        for _ in range(args.rounds):
            for v in variants:
                samples[v[0]].append(time_ms(v[index], args.iters))
        for impl, vals in samples.items():
            row[f"{which}_{impl}_ms"] = statistics.median(vals)
            row[f"{which}_{impl}_min_ms"] = min(vals)
            row[f"{which}_{impl}_max_ms"] = max(vals)
        row[f"{which}_miopen_over_hip"] = (
            row[f"{which}_miopen_ms"] / row[f"{which}_hip_ms"])
    print(json.dumps(row), flush=True)
    return row


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--iters", type=int, default=50)
    parser.add_argument("--rounds", type=int, default=5)
    parser.add_argument("--batches", default="32,512,4096,40960")
    parser.add_argument("--out", default=None, help="markdown table")
    parser.add_argument("--json", default=None, help="raw rows")
    args = parser.parse_args()
    if not t.cuda.is_available():
        raise SystemExit("bench_conv_igemm needs a GPU")
    dev = t.device("cuda:0")
    rows = [bench_layer(name, kwargs, hw, int(b), args, dev)
            for name, kwargs, hw in LAYERS
            for b in args.batches.split(",")]

    def cell(r, key):
        return (f"{r[key + '_ms']:.4f} ({r[key + '_min_ms']:.4f}-"
                f"{r[key + '_max_ms']:.4f})")

    lines = [
        "| layer | N | direction | byte floor ms | hip ms (min-max) | "
        "miopen ms (min-max) | miopen / hip |",
        "|---|---|---|---|---|---|---|",
    ]
    for r in rows:
        for which in ("fwd", "bwd"):
            lines.append(
                f"| {r['layer']} | {r['N']} | {which} | "
                f"{r[which + '_floor_ms']:.4f} | {cell(r, which + '_hip')} | "
                f"{cell(r, which + '_miopen')} | "
                f"{r[which + '_miopen_over_hip']:.2f}x |")
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
