"""Time the IQN cosine tau-embedding: the fused gfx950 kernels against
the torch composition on the device.

    python tools/bench_iqn_embedding.py [--out table.md] [--json rows.json]
        [--batches 32,512] [--quantiles 8,64] [--dims 512,3136]
        [--window 0.25] [--rounds 7]

One call is the forward plus the gradients of ``psi``, ``weight`` and
``bias`` for a given ``dh`` (``taus`` has none), in two forms:

* kernel — ``ops._IQNEmbedding`` (machin_amd/ops/hip/iqn_embed.hip: one
           forward kernel, one backward kernel and the slice reduction);
* torch  — ``ops._iqn_embedding_torch`` on the device.

The forward alone (no autograd) is timed as well; its store bandwidth is
``B N D`` elements of ``h`` over that time.

Method: the two forms are first checked to agree (fp32: rtol 1e-4, atol
1e-4 scaled by the output's largest value; ``dweight`` and ``dbias`` up
to the terms whose ReLU mask is undecided); then each is warmed up and
timed with device events over a window of at least ``--window`` seconds,
``--rounds`` times, alternating the forms inside a round so that clocks
and load are shared; the median round is reported with the min-max
spread. The kernel is "not slower" when it loses by no more than the
rounds' largest min-max spread. Needs a GPU; there is no CPU mode.
Per-kernel device times come from a separate run under a kernel tracer
with ``--window 0.01 --rounds 1``.
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

from machin_amd import ops

K = 64


def make_inputs(B, N, D, dtype, dev):
    gen = t.Generator(device="cpu").manual_seed(B * 7 + N * 3 + D)
    psi = t.randn(B, D, generator=gen).to(dtype).to(dev).requires_grad_(True)
    dh = t.randn(B, N, D, generator=gen).to(dtype).to(dev)
    taus = t.rand(B, N, generator=gen).to(dev)
    weight = ((t.rand(D, K, generator=gen) * 2 - 1) / 8).to(dev)
    bias = ((t.rand(D, generator=gen) * 2 - 1) / 8).to(dev)
    return psi, dh, taus, weight.requires_grad_(True), \
        bias.requires_grad_(True)


def check_equal(got, want, psi, dh, taus, weight, bias):
    """h and dpsi agree to rounding. dweight and dbias also differ by the
    whole term of every element whose ReLU mask ``[z > 0]`` the two forms
    decide differently, which can happen where ``|z| < 1e-5``."""
    N = taus.shape[1]
    with t.no_grad():
        c = t.cos(math.pi * taus.view(-1, 1) * t.arange(K, device=taus.device))
        z = c @ weight.t() + bias
        term = (dh.float().view(-1, dh.shape[-1])
                * psi.float().repeat_interleave(N, dim=0)).abs()
        term = term * (z.abs() < 1e-5)
        slack = (0.0, 0.0, term.t() @ c.abs(), term.sum(dim=0))
        for a, b, s in zip(got, want, slack):
            tol = 1e-4 * b.abs() + 1e-4 * float(b.abs().max()) + s
            assert bool(((a - b).abs() <= tol).all())


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
    forms = {"kernel": ops._IQNEmbedding.apply,
             "torch": ops._iqn_embedding_torch}
    for dtype in (t.float32, t.bfloat16):
        for D in args.dims:
            for N in args.quantiles:
                for B in args.batches:
                    psi, dh, taus, weight, bias = make_inputs(
                        B, N, D, dtype, dev)

                    def step(form):
                        def run():
                            h = form(psi, taus, weight, bias)
                            return (h,) + t.autograd.grad(
                                h, [psi, weight, bias], dh)
                        return run

                    def forward():
                        with t.no_grad():
                            return forms["kernel"](psi, taus, weight, bias)

                    variants = [(n, step(f)) for n, f in forms.items()]
                    variants.append(("kernel_fwd", forward))
                    if dtype == t.float32:
                        check_equal(variants[0][1](), variants[1][1](), psi,
                                    dh, taus, weight, bias)
                    iters = {}
                    for name, fn in variants:
                        per_call = time_ms(fn, 10) / 1e3  # warm-up
                        iters[name] = max(10, math.ceil(args.window / per_call))
                    samples = {name: [] for name, _ in variants}
                    for _ in range(args.rounds):
                        for name, fn in variants:
                            samples[name].append(time_ms(fn, iters[name]))
                    row = {"dtype": str(dtype).split(".")[1], "B": B, "N": N,
                           "D": D, "K": K, "rounds": args.rounds,
                           "window_s": args.window}
                    for name, vals in samples.items():
                        row[name + "_ms"] = statistics.median(vals)
                        row[name + "_min_ms"] = min(vals)
                        row[name + "_max_ms"] = max(vals)
                    row["torch_over_kernel"] = \
                        row["torch_ms"] / row["kernel_ms"]
                    spread = max(row[n + "_max_ms"] - row[n + "_min_ms"]
                                 for n in forms)
                    row["kernel_not_slower"] = \
                        row["kernel_ms"] <= row["torch_ms"] + spread
                    row["fwd_store_GBps"] = B * N * D * psi.element_size() \
                        / (row["kernel_fwd_ms"] * 1e-3) / 1e9
                    rows.append(row)
                    print(json.dumps(row), flush=True)
    return rows


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--window", type=float, default=0.25)
    parser.add_argument("--rounds", type=int, default=7)
    parser.add_argument("--batches", default="32,512")
    parser.add_argument("--quantiles", default="8,64")
    parser.add_argument("--dims", default="512,3136")
    parser.add_argument("--out", default=None, help="markdown table")
    parser.add_argument("--json", default=None, help="raw rows")
    args = parser.parse_args()
    for name in ("batches", "quantiles", "dims"):
        setattr(args, name, [int(v) for v in getattr(args, name).split(",")])
    if not t.cuda.is_available():
        raise SystemExit("bench_iqn_embedding needs a GPU")
    rows = bench(args, t.device("cuda:0"))

    def cell(r, name):
        return (f"{r[name + '_ms']:.4f} ({r[name + '_min_ms']:.4f}-"
                f"{r[name + '_max_ms']:.4f})")

    lines = [
        "| psi | B | N | D | kernel ms (min-max) | torch ms (min-max) | "
        "torch / kernel | kernel not slower | forward ms | h store GB/s |",
        "|---|---|---|---|---|---|---|---|---|---|",
    ]
    for r in rows:
        lines.append(
            f"| {r['dtype']} | {r['B']} | {r['N']} | {r['D']} | "
            f"{cell(r, 'kernel')} | {cell(r, 'torch')} | "
            f"{r['torch_over_kernel']:.2f}x | "
            f"{'yes' if r['kernel_not_slower'] else 'no'} | "
            f"{r['kernel_fwd_ms']:.4f} | {r['fwd_store_GBps']:.0f} |"
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
