"""Time conv2 and conv3 of the Nature CNN, forward and backward apart:
the implicit-GEMM kernels (``impl="hip"``, and ``impl="hip_wrw"`` with
the hand-written weight gradient) against the library composition
(``impl="miopen"``); and the weight gradient alone.

    python tools/bench_conv_igemm.py [--out table.md] [--json rows.json]
        [--batches 32,512,4096,40960] [--iters 50] [--rounds 5]

For ``ConvBiasReLU2d(32, 64, 4, stride=2)`` on 20x20 inputs and
``ConvBiasReLU2d(64, 64, 3, stride=1, flatten=True)`` on 9x9 inputs,
bf16 parameters and channels-last bf16 ``x``:

* forward  — ``y = conv(x)`` (conv + bias + ReLU);
* backward — gradients of ``x``, weight and bias for a given ``dy`` on
             a graph built once (ReLU mask + bias gradient, data
             gradient, weight gradient; the weight gradient is the
             library's except in ``hip_wrw``);
* wrw      — the weight gradient alone on the same ``g`` and ``x``:
             ``ext.conv_igemm_wrw`` (``hip_wrw``) against
             ``aten.convolution_backward`` (``miopen``).

Method: each form runs 10 times first, which also lets the library
finish choosing its algorithms; then it is timed with device events over
``--iters`` calls, ``--rounds`` times, the forms alternating inside a
round so that clocks and load are shared; the median round is reported
with the min-max spread. The byte floor is the activation traffic of the
direction (forward: x in, y out; backward: dy and y in, g out and read
back once, x in, dx out; wrw: g and x in once each) at 5.5 TB/s. Needs a GPU; there is no CPU mode."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(
    0, os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
)

import torch as t

from machin_amd.ops import _require_ext
from machin_amd.ops.fused_conv import ConvBiasReLU2d

# name, module arguments, input H = W
LAYERS = (
    ("conv2", dict(in_channels=32, out_channels=64, kernel_size=4, stride=2),
     20),
    ("conv3", dict(in_channels=64, out_channels=64, kernel_size=3, stride=1,
                   flatten=True), 9),
)
IMPLS = ("hip_wrw", "hip", "miopen")
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
    # the weight gradient alone, both on the same g and x
    k, stride = kwargs["kernel_size"], kwargs["stride"]
    g = t.randn(batch, ohw, ohw, cout, generator=gen).to(dev, t.bfloat16)
    x_rows, g_nchw = x.detach().permute(0, 2, 3, 1), g.permute(0, 3, 1, 2)
    weight = conv.weight.detach()  # only its shape matters
    ext = _require_ext()
    wrw = (
        ("hip_wrw", lambda: ext.conv_igemm_wrw(g, x_rows, k, stride)),
        ("miopen", lambda: t.ops.aten.convolution_backward(
            g_nchw, x.detach(), weight, None, [stride, stride], [0, 0],
            [1, 1], False, [0, 0], 1, [False, True, False])),
    )
    row["wrw_floor_ms"] = batch * (act_in + act_out) / HBM_BYTES_PER_MS
    for which, index in (("fwd", 1), ("bwd", 2), ("wrw", 1)):
        if which == "wrw":
            variants = wrw
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
        for impl in samples:
            if impl != "miopen":
                row[f"{which}_miopen_over_{impl}"] = (
                    row[f"{which}_miopen_ms"] / row[f"{which}_{impl}_ms"])
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
        "| layer | N | direction | byte floor ms | hip_wrw ms (min-max) | "
        "hip ms (min-max) | miopen ms (min-max) | miopen / hip_wrw | "
        "miopen / hip |",
        "|---|---|---|---|---|---|---|---|---|",
    ]
    for r in rows:
        for which in ("fwd", "bwd", "wrw"):
            hip = which != "wrw"  # the wrw rows have no "hip" form
            lines.append(
                f"| {r['layer']} | {r['N']} | {which} | "
                f"{r[which + '_floor_ms']:.4f} | "
                f"{cell(r, which + '_hip_wrw')} | "
                f"{cell(r, which + '_hip') if hip else '-'} | "
                f"{cell(r, which + '_miopen')} | "
                f"{r[which + '_miopen_over_hip_wrw']:.2f}x | "
                + (f"{r[which + '_miopen_over_hip']:.2f}x |" if hip
                   else "- |"))
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
