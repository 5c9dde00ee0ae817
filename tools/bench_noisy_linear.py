"""Time NoisyLinear: the fused gfx950 kernels against the two eager forms,
and the noise kernel against the torch chain.

    python tools/bench_noisy_linear.py [--out table.md] [--json rows.json]
        [--batches 32,512,4096] [--iters 200] [--rounds 7]

For the layers of the Rainbow pixel net (``3136->512``, ``512->306``,
``512->51``), B in {32, 512, 4096} and fp32 / bf16 ``x``, forward plus
backward (gradients of x and of the four parameters for a given ``dy``)
is timed on the GPU in three forms:

* fused    — ``ops._NoisyLinear`` (machin_amd/ops/hip/noisy_linear.hip:
             forward, input-gradient and weight-gradient kernels, plus
             the slice reduction where the reduction is split), at
             every B, whatever ``ops.NOISY_LINEAR_FUSED_MAX_BATCH`` is;
* composed — eager ``W = mu + sigma * outer(eps_out, eps_in)`` and
             ``F.linear(x, W, b)``;
* two_gemm — ``ops._noisy_linear_torch`` on the device:
             ``x @ mu.T + ((x * eps_in) @ sigma.T) * eps_out + b``.

Then ``reset_noise`` on a ``NoisyDuelingC51Head(512, 6, 51)`` (4 layers,
one ``ops.factorised_noise_`` launch each) is timed against the torch
chain ``randn, sign, abs, sqrt, mul`` per noise vector (8 vectors, 40
launches).

Method: the forms are first checked to agree (fp32 ``x``: rtol 1e-4,
atol 1e-4 scaled by the output's largest value); then each is warmed up
and timed with device events over ``--iters`` calls, ``--rounds`` times,
alternating the forms inside a round so that clocks and load are shared;
the median round is reported with the min-max spread. Needs a GPU; there
is no CPU mode. Per-kernel device times come from a separate run under a
kernel tracer with ``--batches 32 --iters 20 --rounds 1``.
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
import torch.nn.functional as F

from machin_amd import ops
from machin_amd.model.nets import NoisyDuelingC51Head, noisy_layers, \
    reset_noise

LAYERS = ((3136, 512), (512, 306), (512, 51))
FORMS = ("fused", "composed", "two_gemm")


def composed(x, mu, sigma, bias_mu, bias_sigma, eps_in, eps_out):
    w = mu + sigma * t.outer(eps_out, eps_in)
    b = bias_mu + bias_sigma * eps_out
    return F.linear(x.float(), w, b).to(x.dtype)


def f_noise(z):
    return z.sign() * z.abs().sqrt()


def make_inputs(B, I, O, dtype, dev):
    gen = t.Generator(device="cpu").manual_seed(B * 7 + I + O)
    bound = 1.0 / I ** 0.5
    x = t.randn(B, I, generator=gen).to(dtype).to(dev).requires_grad_(True)
    dy = t.randn(B, O, generator=gen).to(dtype).to(dev)
    params = [
        ((t.rand(O, I, generator=gen) * 2 - 1) * bound),
        t.full((O, I), 0.5 * bound),
        ((t.rand(O, generator=gen) * 2 - 1) * bound),
        t.full((O,), 0.5 * bound),
    ]
    params = [p.to(dev).requires_grad_(True) for p in params]
    eps = [f_noise(t.randn(n, generator=gen)).to(dev) for n in (I, O)]
    return x, dy, params, eps


def time_ms(fn, iters):
    start = t.cuda.Event(enable_timing=True)
    stop = t.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def summarise(row, samples):
    for name, vals in samples.items():
        row[name + "_ms"] = statistics.median(vals)
        row[name + "_min_ms"] = min(vals)
        row[name + "_max_ms"] = max(vals)


def bench_layers(args, dev):
    rows = []
    forms = {"fused": ops._NoisyLinear.apply, "composed": composed,
             "two_gemm": ops._noisy_linear_torch}
    for dtype in (t.float32, t.bfloat16):
        for I, O in LAYERS:
            for B in args.batches:
                x, dy, params, eps = make_inputs(B, I, O, dtype, dev)

                def step(form):
                    def run():
                        y = form(x, *params, *eps)
                        return (y,) + t.autograd.grad(y, [x] + params, dy)
                    return run

                variants = [(name, step(forms[name])) for name in FORMS]
                if dtype == t.float32:
                    want = variants[0][1]()
                    for _, fn in variants[1:]:
                        for a, b in zip(fn(), want):
                            atol = 1e-4 * float(b.abs().max())
                            assert t.allclose(a, b, rtol=1e-4, atol=atol)
                for _, fn in variants:
                    time_ms(fn, 10)  # warm-up
                samples = {name: [] for name, _ in variants}
                for _ in range(args.rounds):
                    for name, fn in variants:
                        samples[name].append(time_ms(fn, args.iters))
                row = {"dtype": str(dtype).split(".")[1], "I": I, "O": O,
                       "B": B, "iters": args.iters, "rounds": args.rounds}
                summarise(row, samples)
                best = min(row["composed_ms"], row["two_gemm_ms"])
                row["best_eager_over_fused"] = best / row["fused_ms"]
                # fused is "not slower" when it loses by no more than
                # the rounds' min-max spread
                spread = max(
                    row[n + "_max_ms"] - row[n + "_min_ms"] for n in FORMS
                )
                row["fused_not_slower"] = row["fused_ms"] <= best + spread
                rows.append(row)
                print(json.dumps(row), flush=True)
    return rows


def bench_noise(args, dev):
    head = NoisyDuelingC51Head(512, 6, 51).to(dev)
    buffers = [v for layer in noisy_layers(head)
               for v in (layer.eps_in, layer.eps_out)]

    def kernel():
        reset_noise(head)

    def torch_chain():
        for buf in buffers:
            z = t.randn(buf.shape, device=dev)
            t.mul(z.sign(), z.abs().sqrt(), out=buf)

    variants = [("kernel", kernel), ("torch_chain", torch_chain)]
    for _, fn in variants:
        time_ms(fn, 10)
    samples = {name: [] for name, _ in variants}
    for _ in range(args.rounds):
        for name, fn in variants:
            samples[name].append(time_ms(fn, args.iters))
    row = {"what": "reset_noise, NoisyDuelingC51Head(512, 6, 51)",
           "kernel_launches": len(noisy_layers(head)),
           "torch_chain_launches": 5 * len(buffers),
           "iters": args.iters, "rounds": args.rounds}
    summarise(row, samples)
    print(json.dumps(row), flush=True)
    return row


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--iters", type=int, default=200)
    parser.add_argument("--rounds", type=int, default=7)
    parser.add_argument("--batches", default="32,512,4096")
    parser.add_argument("--out", default=None, help="markdown table")
    parser.add_argument("--json", default=None, help="raw rows")
    args = parser.parse_args()
    args.batches = [int(b) for b in args.batches.split(",")]
    if not t.cuda.is_available():
        raise SystemExit("bench_noisy_linear needs a GPU")
    dev = t.device("cuda:0")

    rows = bench_layers(args, dev)
    noise = bench_noise(args, dev)

    def cell(r, name):
        return (f"{r[name + '_ms']:.4f} ({r[name + '_min_ms']:.4f}-"
                f"{r[name + '_max_ms']:.4f})")

    lines = [
        "| x | layer | B | fused ms (min-max) | composed ms | two-GEMM ms | "
        "best eager / fused | fused not slower |",
        "|---|---|---|---|---|---|---|---|",
    ]
    for r in rows:
        lines.append(
            f"| {r['dtype']} | {r['I']}->{r['O']} | {r['B']} | "
            f"{cell(r, 'fused')} | {cell(r, 'composed')} | "
            f"{cell(r, 'two_gemm')} | {r['best_eager_over_fused']:.2f}x | "
            f"{'yes' if r['fused_not_slower'] else 'no'} |"
        )
    lines += [
        "",
        "| noise resampling | launches | ms (min-max) |",
        "|---|---|---|",
        f"| reset_noise (kernel) | {noise['kernel_launches']} | "
        f"{cell(noise, 'kernel')} |",
        f"| torch chain | {noise['torch_chain_launches']} | "
        f"{cell(noise, 'torch_chain')} |",
    ]
    table = "\n".join(lines)
    print(table)
    if args.out:
        with open(args.out, "w") as f:
            f.write(table + "\n")
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"layers": rows, "noise": noise}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
