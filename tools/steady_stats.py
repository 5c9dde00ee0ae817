"""Aggregate a rocprofv3 kernel trace over only its FINAL time window
(default last 25%), excluding the MIOpen/cudnn-benchmark autotune
find-phase that pollutes whole-run stats (round-1 VERDICT weak #7).

Usage: python tools/steady_stats.py <kernel_trace.csv> [anchor]
           [n_steps] [out.md] [--full-names] [--by-grid] [--top N]

``--full-names`` keeps the whole demangled kernel name (the default
cuts at the first "(" and at 80 characters, which makes every ATen
``vectorized_elementwise_kernel<8, ...>`` instantiation look alike);
``--by-grid`` additionally splits each kernel by its launch grid, so
the same elementwise kernel run on tensors of different sizes shows up
as separate rows and can be attributed by bytes.
"""
import collections
import csv
import sys


def main():
    argv = list(sys.argv[1:])
    full_names = "--full-names" in argv
    by_grid = "--by-grid" in argv
    top = 25
    if "--top" in argv:
        i = argv.index("--top")
        top = int(argv[i + 1])
        del argv[i:i + 2]
    argv = [a for a in argv if a not in ("--full-names", "--by-grid")]
    path = argv[0]
    anchor = argv[1] if len(argv) > 1 else "conv1_fwd"
    n_steps = int(argv[2]) if len(argv) > 2 else 30
    out_md = argv[3] if len(argv) > 3 else None
    rows = list(csv.DictReader(open(path)))
    skey = next(k for k in rows[0] if "Start" in k)
    ekey = next(k for k in rows[0] if "End" in k)
    nkey = next(k for k in rows[0] if "Kernel_Name" in k or "Name" in k)
    gkey = next((k for k in rows[0] if k.startswith("Grid_Size")), None)
    # anchor the steady window on the last n_steps dispatches of a
    # once-per-step kernel: immune to autotune kernels interleaved
    # anywhere else in the trace
    anchors = sorted(
        int(r[skey]) for r in rows if anchor in r[nkey]
    )
    if len(anchors) < n_steps + 1:
        raise SystemExit(f"only {len(anchors)} {anchor!r} dispatches")
    cut = anchors[-n_steps]
    t1 = max(int(r[ekey]) for r in rows)
    t0 = cut
    frac = n_steps
    # calls, total ms, min ms, max ms of one dispatch
    agg = collections.defaultdict(lambda: [0, 0.0, float("inf"), 0.0])
    total = 0.0
    for r in rows:
        if int(r[skey]) < cut:
            continue
        dur = (int(r[ekey]) - int(r[skey])) / 1e6
        if full_names:
            name = r[nkey].strip()
        else:
            name = r[nkey].split("(")[0].strip()[:80]
        if by_grid and gkey is not None:
            gx = gkey if gkey.endswith("_X") else None
            grid = r[gx] if gx else r[gkey]
            name = f"{name} [grid {grid}]"
        agg[name][0] += 1
        agg[name][1] += dur
        agg[name][2] = min(agg[name][2], dur)
        agg[name][3] = max(agg[name][3], dur)
        total += dur
    lines = [
        f"# Steady-state kernel profile: window = last {n_steps} "
        f"dispatches of '{anchor}' ({(t1 - t0) / 1e6:.0f} ms; MIOpen "
        f"autotune/find phases outside the window are EXCLUDED)",
        "",
        "| % | total ms | calls | avg ms | min ms | max ms | kernel |",
        "|---|---|---|---|---|---|---|",
    ]
    for name, (calls, ms, lo, hi) in sorted(
        agg.items(), key=lambda kv: -kv[1][1]
    )[:top]:
        lines.append(
            f"| {ms / total * 100:5.1f} | {ms:9.2f} | {calls:5d} | "
            f"{ms / calls:7.3f} | {lo:7.3f} | {hi:7.3f} | `{name}` |"
        )
    text = "\n".join(lines) + "\n"
    print(text)
    if out_md:
        with open(out_md, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
