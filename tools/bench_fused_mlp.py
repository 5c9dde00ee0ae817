"""Time the whole-network fused MLP: the gfx950 kernels against the torch
forms on the device.

    python tools/bench_fused_mlp.py [--out table.md] [--json rows.json]
        [--batches 1,32,256,1024,4096] [--window 0.25] [--rounds 7]

Nets: ``4 -> 64 -> 64 -> 2``, ``17 -> 256 -> 256 -> 6`` and an ensemble
of two ``23 -> 256 -> 256 -> 1`` on a shared ``x`` (twin critics). For
each net and batch, two calls in two forms:

* forward           — under ``no_grad``;
* forward + backward — the forward plus the gradients of ``x``, every
                      weight and every bias for a given ``dy``;
* kernel — ``ops._FusedMLP`` (machin_amd/ops/hip/fused_mlp.hip: one
           kernel forward, two backward, plus the member sum of ``dx``
           for the ensemble);
* torch  — an ``nn.Linear`` / ReLU chain for a single net,
           ``ops._fused_mlp_torch`` (``baddbmm``) for the ensemble.

Method: the two forms are first checked to agree (rtol 1e-4, atol 1e-4
scaled by the output's largest value); then each is warmed up and timed
with device events over a window of at least ``--window`` seconds,
``--rounds`` times, alternating the forms inside a round so that clocks
and load are shared; the median round is reported with the min-max
spread. The kernel "wins" when its median is below the torch form's.
Needs a GPU; there is no CPU mode.
"""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(
    0, os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
)

import torch as t
import torch.nn.functional as F

from machin_amd import ops
from machin_amd.model.nets import FusedMLP

NETS = [(None, (4, 64, 64, 2)), (None, (17, 256, 256, 6)),
        (2, (23, 256, 256, 1))]


def linear_chain(x, weights, biases):
    for w, b in zip(weights[:-1], biases[:-1]):
        x = t.relu(F.linear(x, w, b))
    return F.linear(x, weights[-1], biases[-1])


def kernel_form(x, weights, biases):
    """ops.fused_mlp without its batch limit."""
    if weights[0].dim() == 3:
        return ops._FusedMLP.apply(x, len(weights), *weights, *biases)
    return ops._FusedMLP.apply(
        x.unsqueeze(0), len(weights), *[w.unsqueeze(0) for w in weights],
        *[b.unsqueeze(0) for b in biases]).squeeze(0)


def time_ms(fn, iters):
    start = t.cuda.Event(enable_timing=True)
    stop = t.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def bench(args, dev):
    rows = []
    for E, sizes in NETS:
        t.manual_seed(sum(sizes))
        net = FusedMLP(sizes, ensemble=E).to(dev)
        weights, biases = list(net.weights), list(net.biases)
        torch_form = linear_chain if E is None else ops._fused_mlp_torch
        for B in args.batches:
            gen = t.Generator(device="cpu").manual_seed(B)
            x = t.randn(B, sizes[0], generator=gen).to(dev)
            x.requires_grad_(True)
            lead = () if E is None else (E,)
            dy = t.randn(*lead, B, sizes[-1], generator=gen).to(dev)

            def step(form):
                def run():
                    y = form(x, weights, biases)
                    return (y,) + t.autograd.grad(
                        y, [x] + weights + biases, dy)
                return run

            def forward(form):
                def run():
                    with t.no_grad():
                        return form(x, weights, biases)
                return run

            variants = [("kernel", step(kernel_form)),
                        ("torch", step(torch_form)),
                        ("kernel_fwd", forward(kernel_form)),
                        ("torch_fwd", forward(torch_form))]
            for a, b in zip(variants[0][1](), variants[1][1]()):
                tol = 1e-4 * b.abs() + 1e-4 * float(b.abs().max())
                assert bool(((a - b).abs() <= tol).all())
            iters = {}
            for name, fn in variants:
                per_call = time_ms(fn, 10) / 1e3  # warm-up
                iters[name] = max(10, math.ceil(args.window / per_call))
            samples = {name: [] for name, _ in variants}
            for _ in range(args.rounds):
                for name, fn in variants:
                    samples[name].append(time_ms(fn, iters[name]))
            row = {"E": E, "sizes": list(sizes), "B": B,
                   "rounds": args.rounds, "window_s": args.window}
            for name, vals in samples.items():
                row[name + "_ms"] = statistics.median(vals)
                row[name + "_min_ms"] = min(vals)
                row[name + "_max_ms"] = max(vals)
            row["fwd_torch_over_kernel"] = \
                row["torch_fwd_ms"] / row["kernel_fwd_ms"]
            row["torch_over_kernel"] = row["torch_ms"] / row["kernel_ms"]
            row["kernel_wins"] = row["kernel_ms"] < row["torch_ms"]
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--window", type=float, default=0.25)
    parser.add_argument("--rounds", type=int, default=7)
    parser.add_argument("--batches", default="1,32,256,1024,4096")
    parser.add_argument("--out", default=None, help="markdown table")
    parser.add_argument("--json", default=None, help="raw rows")
    args = parser.parse_args()
    args.batches = [int(v) for v in args.batches.split(",")]
    if not t.cuda.is_available():
        raise SystemExit("bench_fused_mlp needs a GPU")
    rows = bench(args, t.device("cuda:0"))

    def cell(r, name):
        return (f"{r[name + '_ms']:.4f} ({r[name + '_min_ms']:.4f}-"
                f"{r[name + '_max_ms']:.4f})")

    lines = [
        "| net | B | forward: kernel ms (min-max) | forward: torch ms | "
        "torch / kernel | fwd + bwd: kernel ms (min-max) | "
        "fwd + bwd: torch ms | torch / kernel | kernel wins |",
        "|---|---|---|---|---|---|---|---|---|",
    ]
    for r in rows:
        net = " -> ".join(str(s) for s in r["sizes"])
        if r["E"] is not None:
            net = f"E = {r['E']}, {net}, shared x"
        lines.append(
            f"| {net} | {r['B']} | {cell(r, 'kernel_fwd')} | "
            f"{cell(r, 'torch_fwd')} | {r['fwd_torch_over_kernel']:.2f}x | "
            f"{cell(r, 'kernel')} | {cell(r, 'torch')} | "
            f"{r['torch_over_kernel']:.2f}x | "
            f"{'yes' if r['kernel_wins'] else 'no'} |"
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
