"""Time the frame-stack gather of the frame-deduplicated replay.

    python tools/bench_framestack.py [--out table.md] [--n-step N]
        [--shift PAD]

For 84x84 frames, k=4 and B in {32, 512, 4096}, in both output
layouts, three ways of producing one sampled (state, next_state)
batch are timed on the GPU:

* kernel   — ``ops.framestack_gather`` (one gfx950 kernel);
* torch    — the same result as a torch composition over the SAME
             frame ring (index matrix, ``index_select``, two slices,
             two layout copies);
* stacked  — what ``DeviceTransitionBuffer`` does: ``index_select``
             from two pre-stacked ``[N, 4, 84, 84]`` rings (for the
             NHWC rows plus the two ``channels_last`` copies needed
             to hand the batch to the fused u8 conv stem).

Method: all three are checked to return the same bytes first; then
each is warmed up and timed with device events over ``--iters`` calls,
``--rounds`` times, alternating the three variants inside a round; the
median round is reported with the min-max spread. Indices are fresh
random draws per call from a ring larger than the 256 MiB Infinity
Cache, as in a real replay. Needs a GPU; there is no CPU mode.

With ``--n-step N`` (N > 1) the table is about
``ops.framestack_gather_nstep`` instead, same shapes and method, on a
transition ring of ``--frames`` rows cut into episodes of 1000 steps
(so nearly every window has m = N):

* nstep kernel — ``ops.framestack_gather_nstep`` (one gfx950 kernel);
* nstep torch  — the same result as a torch composition over the same
                 rings (``ops._framestack_gather_nstep_torch``);
* 1-step kernel — ``ops.framestack_gather`` on the same draws (the
                 base column is the identity, so ``base[pos]`` is
                 ``pos``), timed in the same rounds: the n-step
                 kernel's ratio to it is printed next to the ratio of
                 the plane bytes the two must move.

With ``--shift PAD`` (PAD > 0) the table is about the random-shift
augmentation fused into the gather (``shift=``), same shapes and
method, one int32 ``[B, 4]`` draw uniform on ``[-PAD, PAD]`` per call;
with ``--n-step N`` as well it is about the n-step op:

* shifted kernel    — the op with ``shift=`` (one gfx950 kernel);
* un-shifted kernel — the op without it on the same draws (equal plane
                      bytes), timed in the same rounds: the ratio of the
                      two is printed next to the max / min spread of the
                      un-shifted kernel's rounds;
* torch composition — ``ops._framestack_gather_shift_torch`` (or the
                      n-step one) on the device: the un-shifted torch
                      composition plus one advanced-index gather per
                      stack, what a user would otherwise run.
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

H = W = 84
K = 4


def stored_bytes(episode_len: int):
    """Bytes of HBM per stored transition for the frame columns (plus
    the int64 base-slot column of the frame ring)."""
    stacked = 2 * K * H * W
    dedup = H * W * (episode_len + K) / episode_len + 8
    return stacked, dedup


def time_ms(fn, draws, iters):
    start = t.cuda.Event(enable_timing=True)
    stop = t.cuda.Event(enable_timing=True)
    start.record()
    for i in range(iters):
        fn(draws[i % len(draws)])
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def nstep_table(args, dev):
    """Rows for ops.framestack_gather_nstep (see the module docstring)."""
    n, gamma, L = args.n_step, 0.99, 1000
    P = T = args.frames
    ring = t.randint(0, 256, (P, H, W), dtype=t.uint8, device=dev)
    base = t.arange(T, device=dev)
    left = (L - 1) - t.arange(T, device=dev) % L
    reward = t.randn(T, device=dev)
    terminal = (left == 0).float()
    m = min(n, K)
    # plane bytes: k + min(m, k) reads and 2k writes, against k+1 and 2k
    nstep_planes, one_planes = 3 * K + m, 3 * K + 1

    rows = []
    for nhwc in (False, True):
        def nstep_kernel(pos):
            return ops.framestack_gather_nstep(
                ring, base, left, reward, terminal, pos, K, n, gamma, nhwc)

        def nstep_torch(pos):
            return ops._framestack_gather_nstep_torch(
                ring, base, left, reward, terminal, pos, K, n, gamma, nhwc)

        def one_step_kernel(pos):
            # base is the identity here, so base[pos] == pos
            return ops.framestack_gather(ring, pos, K, nhwc)

        variants = [("nstep", nstep_kernel), ("torch", nstep_torch),
                    ("onestep", one_step_kernel)]
        for B in (32, 512, 4096):
            draws = [t.randint(0, T, (B,), device=dev) for _ in range(16)]
            want, got = nstep_kernel(draws[0]), nstep_torch(draws[0])
            for i in (0, 1, 3, 4):
                assert t.equal(got[i], want[i])
                assert got[i].stride() == want[i].stride()
            assert t.allclose(got[2], want[2], rtol=1e-5, atol=1e-6)
            for _, fn in variants:
                time_ms(fn, draws, 20)  # warm-up
            samples = {name: [] for name, _ in variants}
            for _ in range(args.rounds):
                for name, fn in variants:
                    samples[name].append(time_ms(fn, draws, args.iters))
            row = {"layout": "nhwc" if nhwc else "nchw", "B": B, "n": n}
            for name, vals in samples.items():
                row[name + "_ms"] = statistics.median(vals)
                row[name + "_min_ms"] = min(vals)
                row[name + "_max_ms"] = max(vals)
            row["nstep_GBps"] = (
                B * nstep_planes * H * W / (row["nstep_ms"] * 1e-3) / 1e9
            )
            rows.append(row)
            print(json.dumps(row), flush=True)

    lines = [
        f"| layout | B | n-step kernel ms (min-max), n={n} | "
        "torch, same rings ms | 1-step kernel ms (min-max) | "
        "n-step kernel GB/s | torch / n-step kernel | "
        f"n-step / 1-step kernel (bytes: {nstep_planes}/{one_planes} = "
        f"{nstep_planes / one_planes:.3f}) |",
        "|---|---|---|---|---|---|---|---|",
    ]
    for r in rows:
        lines.append(
            f"| {r['layout']} | {r['B']} | {r['nstep_ms']:.4f} "
            f"({r['nstep_min_ms']:.4f}-{r['nstep_max_ms']:.4f}) | "
            f"{r['torch_ms']:.4f} "
            f"({r['torch_min_ms']:.4f}-{r['torch_max_ms']:.4f}) | "
            f"{r['onestep_ms']:.4f} "
            f"({r['onestep_min_ms']:.4f}-{r['onestep_max_ms']:.4f}) | "
            f"{r['nstep_GBps']:.0f} | "
            f"{r['torch_ms'] / r['nstep_ms']:.2f}x | "
            f"{r['nstep_ms'] / r['onestep_ms']:.3f} |"
        )
    lines.append("")
    for L in (100, 1000):
        stacked_b, dedup_b = stored_bytes(L)
        lines.append(
            f"RAINBOW frame bytes per stored transition, episodes of {L} "
            f"steps: host fold into stacked rings {stacked_b}, raw "
            f"episodes in the frame ring {dedup_b + 8:.0f} with the two "
            f"int64 columns ({stacked_b / (dedup_b + 8):.2f}x)."
        )
    return lines


def shift_table(args, dev):
    """Rows for the shifted gathers (see the module docstring)."""
    pad, n, gamma, L = args.shift, args.n_step, 0.99, 1000
    P = T = args.frames
    ring = t.randint(0, 256, (P, H, W), dtype=t.uint8, device=dev)
    base = t.arange(T, device=dev)
    left = (L - 1) - t.arange(T, device=dev) % L
    reward = t.randn(T, device=dev)
    terminal = (left == 0).float()
    # plane bytes: the shift moves the bytes of the un-shifted kernel
    planes = 3 * K + (min(n, K) if n > 1 else 1)

    def gather(pos, nhwc, shift, torch_form=False):
        if n > 1:
            if torch_form:
                return ops._framestack_gather_nstep_shift_torch(
                    ring, base, left, reward, terminal, pos, K, n, gamma,
                    nhwc, shift)
            return ops.framestack_gather_nstep(
                ring, base, left, reward, terminal, pos, K, n, gamma, nhwc,
                shift=shift)
        # base is the identity here, so base[pos] == pos
        if torch_form:
            return ops._framestack_gather_shift_torch(ring, pos, K, nhwc,
                                                      shift)
        return ops.framestack_gather(ring, pos, K, nhwc, shift=shift)

    rows = []
    for nhwc in (False, True):
        variants = [
            ("shift", lambda d: gather(d[0], nhwc, d[1])),
            ("plain", lambda d: gather(d[0], nhwc, None)),
            ("torch", lambda d: gather(d[0], nhwc, d[1], True)),
        ]
        for B in (32, 512, 4096):
            draws = [
                (t.randint(0, T, (B,), device=dev),
                 t.randint(-pad, pad + 1, (B, 4), dtype=t.int32,
                           device=dev))
                for _ in range(16)
            ]
            pos, shift = draws[0]
            want, got = gather(pos, nhwc, shift), gather(pos, nhwc, shift,
                                                         True)
            zero = gather(pos, nhwc, t.zeros_like(shift))
            plain = gather(pos, nhwc, None)
            for i in range(2):
                assert t.equal(got[i], want[i])
                assert got[i].stride() == want[i].stride()
                assert t.equal(zero[i], plain[i])
            for _, fn in variants:
                time_ms(fn, draws, 20)  # warm-up
            samples = {name: [] for name, _ in variants}
            for _ in range(args.rounds):
                for name, fn in variants:
                    samples[name].append(time_ms(fn, draws, args.iters))
            row = {"layout": "nhwc" if nhwc else "nchw", "B": B, "n": n,
                   "pad": pad}
            for name, vals in samples.items():
                row[name + "_ms"] = statistics.median(vals)
                row[name + "_min_ms"] = min(vals)
                row[name + "_max_ms"] = max(vals)
            row["shift_GBps"] = (
                B * planes * H * W / (row["shift_ms"] * 1e-3) / 1e9
            )
            rows.append(row)
            print(json.dumps(row), flush=True)

    what = f"n-step (n={n})" if n > 1 else "1-step"
    lines = [
        f"| layout | B | shifted {what} kernel ms (min-max), pad={pad} | "
        "un-shifted kernel, same draws ms (min-max) | "
        "torch composition ms | shifted kernel GB/s | "
        "torch / shifted | shifted / un-shifted | "
        "un-shifted max / min |",
        "|---|---|---|---|---|---|---|---|---|",
    ]
    for r in rows:
        lines.append(
            f"| {r['layout']} | {r['B']} | {r['shift_ms']:.4f} "
            f"({r['shift_min_ms']:.4f}-{r['shift_max_ms']:.4f}) | "
            f"{r['plain_ms']:.4f} "
            f"({r['plain_min_ms']:.4f}-{r['plain_max_ms']:.4f}) | "
            f"{r['torch_ms']:.4f} "
            f"({r['torch_min_ms']:.4f}-{r['torch_max_ms']:.4f}) | "
            f"{r['shift_GBps']:.0f} | "
            f"{r['torch_ms'] / r['shift_ms']:.2f}x | "
            f"{r['shift_ms'] / r['plain_ms']:.3f} | "
            f"{r['plain_max_ms'] / r['plain_min_ms']:.3f} |"
        )
    return lines


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--frames", type=int, default=65536,
                        help="planes in the frame ring (462 MB)")
    parser.add_argument("--transitions", type=int, default=16384,
                        help="rows of each pre-stacked ring (462 MB)")
    parser.add_argument("--iters", type=int, default=1000)
    parser.add_argument("--rounds", type=int, default=7)
    parser.add_argument("--out", default=None)
    parser.add_argument("--n-step", type=int, default=1,
                        help="> 1: time ops.framestack_gather_nstep")
    parser.add_argument("--shift", type=int, default=0, metavar="PAD",
                        help="> 0: time the shifted gathers (random-shift "
                             "augmentation, draws uniform on [-PAD, PAD]); "
                             "combines with --n-step")
    args = parser.parse_args()
    if not t.cuda.is_available():
        raise SystemExit("bench_framestack needs a GPU")
    dev = t.device("cuda:0")
    t.manual_seed(0)
    if args.shift > 0:
        table = "\n".join(shift_table(args, dev))
        print(table)
        if args.out:
            with open(args.out, "w") as f:
                f.write(table + "\n")
        return
    if args.n_step > 1:
        table = "\n".join(nstep_table(args, dev))
        print(table)
        if args.out:
            with open(args.out, "w") as f:
                f.write(table + "\n")
        return

    P, N = args.frames, args.transitions
    ring = t.randint(0, 256, (P, H, W), dtype=t.uint8, device=dev)
    # pre-stacked rings holding the same windows for bases 0..N-1
    all_base = t.arange(N, device=dev)
    st_ring = t.empty((N, K, H, W), dtype=t.uint8, device=dev)
    nx_ring = t.empty_like(st_ring)
    for lo in range(0, N, 2048):
        s, n = ops.framestack_gather(ring, all_base[lo : lo + 2048], K)
        st_ring[lo : lo + 2048], nx_ring[lo : lo + 2048] = s, n

    rows = []
    for nhwc in (False, True):
        fmt = t.channels_last if nhwc else t.contiguous_format

        def kernel(base):
            return ops.framestack_gather(ring, base, K, nhwc)

        def torch_same_ring(base):
            return ops._framestack_gather_torch(ring, base, K, nhwc)

        def stacked(base):
            return (
                st_ring.index_select(0, base).contiguous(
                    memory_format=fmt),
                nx_ring.index_select(0, base).contiguous(
                    memory_format=fmt),
            )

        variants = [("kernel", kernel), ("torch", torch_same_ring),
                    ("stacked", stacked)]
        for B in (32, 512, 4096):
            draws = [t.randint(0, N, (B,), device=dev) for _ in range(16)]
            want = kernel(draws[0])
            for _, fn in variants[1:]:
                got = fn(draws[0])
                assert t.equal(got[0], want[0]) and got[0].stride() == \
                    want[0].stride()
                assert t.equal(got[1], want[1])
            for _, fn in variants:
                time_ms(fn, draws, 20)  # warm-up
            samples = {name: [] for name, _ in variants}
            for _ in range(args.rounds):
                for name, fn in variants:
                    samples[name].append(time_ms(fn, draws, args.iters))
            row = {"layout": "nhwc" if nhwc else "nchw", "B": B}
            for name, vals in samples.items():
                row[name + "_ms"] = statistics.median(vals)
                row[name + "_min_ms"] = min(vals)
                row[name + "_max_ms"] = max(vals)
            # bytes the kernel must move: k+1 plane reads, 2k writes
            row["kernel_GBps"] = (
                B * (3 * K + 1) * H * W / (row["kernel_ms"] * 1e-3) / 1e9
            )
            rows.append(row)
            print(json.dumps(row), flush=True)

    lines = [
        "| layout | B | kernel ms (min-max) | torch, same ring ms | "
        "stacked rings ms | kernel GB/s | torch / kernel | "
        "stacked / kernel |",
        "|---|---|---|---|---|---|---|---|",
    ]
    for r in rows:
        lines.append(
            f"| {r['layout']} | {r['B']} | {r['kernel_ms']:.4f} "
            f"({r['kernel_min_ms']:.4f}-{r['kernel_max_ms']:.4f}) | "
            f"{r['torch_ms']:.4f} "
            f"({r['torch_min_ms']:.4f}-{r['torch_max_ms']:.4f}) | "
            f"{r['stacked_ms']:.4f} "
            f"({r['stacked_min_ms']:.4f}-{r['stacked_max_ms']:.4f}) | "
            f"{r['kernel_GBps']:.0f} | "
            f"{r['torch_ms'] / r['kernel_ms']:.2f}x | "
            f"{r['stacked_ms'] / r['kernel_ms']:.2f}x |"
        )
    lines.append("")
    for L in (100, 1000):
        stacked_b, dedup_b = stored_bytes(L)
        lines.append(
            f"Frame bytes per stored transition, episodes of {L} steps: "
            f"stacked {stacked_b}, frame ring {dedup_b:.0f} "
            f"({stacked_b / dedup_b:.2f}x)."
        )
    table = "\n".join(lines)
    print(table)
    if args.out:
        with open(args.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
