#!/usr/bin/env python
"""Time the grouped Linear4bit launch (ops.int4_linear_grouped) against the loop of per-expert launches it replaces.

Not a test and not bench.py. Routing: 256 experts, top-8, seeded multinomial with the Zipf-skewed popularity of bench.py's C5
(1 / rank^0.8, permuted). Cases: rows = 16384 (a 2048-token step) and 131072 (C5's 16384 tokens), at (K, N) = (7168, 2048) and
(2048, 7168). Per case, in ONE process, the methods alternate round by round on the same tensors:
  grouped        one ops.int4_linear_grouped launch, offsets on the device
  loop           ops.int4_linear per non-empty group on row slices, offsets known on the host beforehand (the loop's best case)
  loop+tolist    the same loop including the ``group_offsets.tolist()`` it needs in real use (a device synchronisation per step)
  loop fp6       ops.int4_linear_fp6 per group with kept weight images (the dense default's matrix path)
A timing is a host clock around `reps` calls that ends in a device synchronise; each round gives one per-call time, and the table shows
the median over the rounds and their spread (min .. max). The outputs of all methods are compared bit for bit first.

Without --case the tool starts every case as a child process of its own under a time limit and stops at the first that fails;
the table goes to profiles/gemm_grouped.txt (--out)."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CASES = [(16384, 7168, 2048), (16384, 2048, 7168), (131072, 7168, 2048), (131072, 2048, 7168)]
EXPERTS, TOPK = 256, 8


def routing(rows, torch):
    """group sizes of rows / TOPK tokens routed top-8 over 256 experts with bench.py C5's popularity law"""
    g = torch.Generator().manual_seed(5)
    pop = 1.0 / torch.arange(1, EXPERTS + 1, dtype=torch.float64) ** 0.8
    indices = torch.multinomial(pop[torch.randperm(EXPERTS, generator=g)].expand(rows // TOPK, EXPERTS), TOPK, replacement=False, generator=g)
    return torch.bincount(indices.flatten(), minlength=EXPERTS)


def run_case(rows, K, N, rounds, out):
    import torch
    from flatquant_amd import ops
    assert torch.cuda.is_available(), "this tool measures on a GPU; there is no CPU path"
    dev = torch.device("cuda", 0)
    counts = routing(rows, torch)
    offsets_host = [0] + torch.cumsum(counts, 0).tolist()
    offsets = torch.tensor(offsets_host, dtype=torch.int64, device=dev)
    gen = torch.Generator(device=dev).manual_seed(rows + K)
    x = torch.randint(0, 256, (rows, K // 2), generator=gen, device=dev, dtype=torch.uint8)
    sx = (torch.rand(rows, generator=gen, device=dev) * 0.05 + 0.001).half()
    w = torch.randint(0, 256, (EXPERTS, N, K // 2), generator=gen, device=dev, dtype=torch.uint8)
    sw = (torch.rand(EXPERTS, N, generator=gen, device=dev) * 0.02 + 0.0005).half()
    images = [ops.int4_to_bf6(w[e], weights=True) for e in range(EXPERTS)]

    def grouped():
        return ops.int4_linear_grouped(x, sx, w, sw, offsets)

    def loop(off=offsets_host, fp6=False):
        ys = []
        for e in range(EXPERTS):
            a, b = off[e], off[e + 1]
            if b > a:
                ys.append(ops.int4_linear_fp6(x[a:b], sx[a:b], w[e], images[e], sw[e]) if fp6 else ops.int4_linear(x[a:b], sx[a:b], w[e], sw[e]))
        return ys

    methods = [("grouped", grouped, 20), ("loop", loop, 4), ("loop+tolist", lambda: loop(offsets.tolist()), 4), ("loop fp6", lambda: loop(fp6=True), 4)]
    want = torch.cat(loop())
    same = {name: bool(torch.equal(y if name == "grouped" else torch.cat(y), want)) for name, fn, _ in methods for y in [fn()]}
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in methods}
    for _ in range(rounds):
        for name, fn, reps in methods:
            fn()                                    # (warm: every shape of the window has run)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / reps * 1e6)
    nonempty = int((counts > 0).sum())
    lines = [f"rows={rows} K={K} N={N}: {EXPERTS} experts, {nonempty} non-empty, largest {int(counts.max())}, median {int(counts.median())} rows; "
             f"{rounds} rounds, us per call: median (min .. max)"]
    med = {k: statistics.median(v) for k, v in times.items()}
    for name, _, reps in methods:
        v = times[name]
        lines.append(f"  {name:<12} {med[name]:10.1f}  ({min(v):.1f} .. {max(v):.1f})  x{reps} calls per round   bits equal to the loop: {same[name]}"
                     + ("" if name == "grouped" else f"   grouped / this = {med['grouped'] / med[name]:.3f}"))
    spread = max((max(v) - min(v)) / statistics.median(v) for v in (times["grouped"], times["loop"]))
    lines.append(f"  grouped / loop = {med['grouped'] / med['loop']:.3f}; run-to-run spread of the two (max - min) / median: {100 * spread:.1f} %")
    text = "\n".join(lines)
    print(text, flush=True)
    with open(out, "a") as f:
        f.write(text + "\n\n")
    return 0 if all(same.values()) else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--case", type=int, nargs=3, metavar=("ROWS", "K", "N"), help="measure one case in this process")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--limit", type=int, default=240, help="seconds a case's process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gemm_grouped.txt"))
    a = ap.parse_args()
    if a.case:
        return run_case(*a.case, a.rounds, a.out)
    with open(a.out, "w") as f:
        f.write("tools/time_gemm_grouped.py: ops.int4_linear_grouped against the per-expert loop; MI355X, one process per case, methods alternating\n\n")
    for rows, K, N in CASES:
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", str(rows), str(K), str(N), "--rounds", str(a.rounds),
                             "--out", a.out], timeout=a.limit).returncode
        if rc != 0:                                  # (a failed or faulted case: nothing more is started on the device)
            print(f"case rows={rows} K={K} N={N} ended with {rc}: stopping", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
