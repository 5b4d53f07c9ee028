#!/usr/bin/env python3
"""The prompt-sized step over the paged INT4 cache (ops.kv_chunk_extend -> fq_kv_chunk_extend) against the launch it relieves
(ops.kv_batch_extend -> fq_kv_batch_extend) on the same cache: Llama-3-8B heads (32 query / 8 KV, head_dim 128), INT4 pages of 16 rows scattered
over the pool, the replicated layout read one copy per KV head and the shared layout; T new tokens per request, the cached rows per request
INCLUDING them.
    tools/time_kv_chunk_extend.py [--shapes 1x2048x16,...] [--layouts replicated,shared] [--out profiles/kv_chunk_extend.txt] [--limit 240]
A shape is REQUESTSxROWSxT. Every (layout, shape) is measured in a child process of its own under a time limit (--limit seconds); a child that
fails or runs out of time ends the run. Figures: the median over rounds of a captured graph of 20 launches (the per-call Python cost is not in
it), the two launches alternating round by round; TFLOP/s counts the causal work, 4 d per (query head, token, visible row). Every launch of a
graph reads the same cache: one request's 2 MB of rows (8 KV heads x 2048 rows x 128 bytes) stay in the caches between launches, which the 32
layers of a model between two launches on one layer would not allow. Read the small shapes as lower bounds, for both launches alike."""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q_HEADS, KV_HEADS, HD, PAGE = 32, 8, 128, 16
TOKENS = (16, 32, 64, 128, 512, 2048)
DEFAULT_SHAPES = [f"{b}x2048x{t}" for b in (1, 8, 64) for t in TOKENS] + ["1x8192x2048"]


def graph_of(torch, fn, steps):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fn()                                       # (eager first: the split workspace exists before the capture)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        for _ in range(steps):
            fn()
    return g


def timed(torch, g, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / steps


def case(layout, bsz, rows, T, rounds=5, steps=20):
    import torch
    sys.path.insert(0, ROOT)
    from flatquant_amd import ops
    g = torch.Generator(device="cuda").manual_seed(0)
    cache_heads, copies = (KV_HEADS, 1) if layout == "shared" else (Q_HEADS, Q_HEADS // KV_HEADS)
    n_pg = rows // PAGE
    data = torch.randint(0, 256, (bsz * n_pg, 1, 2, cache_heads, PAGE, HD // 2), generator=g, device="cuda", dtype=torch.uint8)
    par = (torch.rand(bsz * n_pg, 1, 2, cache_heads, PAGE, 2, generator=g, device="cuda") * 0.2 + 0.05).half()
    indptr = torch.arange(bsz + 1, device="cuda", dtype=torch.int32) * n_pg
    indices = torch.randperm(bsz * n_pg, generator=g, device="cuda").to(torch.int32)
    last = torch.full((bsz,), PAGE, device="cuda", dtype=torch.int32)
    q = (torch.randn(bsz, T, Q_HEADS, HD, generator=g, device="cuda") * 0.5).half()
    new = lambda: ops.kv_chunk_extend(q, data, par, indptr, indices, last, 0, kv_copies=copies)
    old = lambda: ops.kv_batch_extend(q, data, par, indptr, indices, last, 0, seq_hint=rows, kv_copies=copies)
    with torch.no_grad():
        diff = (new().float() - old().float()).abs().max().item()
        graphs = [graph_of(torch, new, steps), graph_of(torch, old, steps)]
        us = [[], []]
        for _ in range(rounds):                                                    # alternately, round by round
            for i, gr in enumerate(graphs):
                us[i].append(timed(torch, gr, steps))
    n, o = (statistics.median(u) for u in us)
    flop = 4.0 * HD * Q_HEADS * bsz * sum(rows - T + t + 1 for t in range(T))
    print(f"{layout:<10s} {bsz:>2d} x {rows:<4d} T={T:<4d} chunk {n:9.1f} us {flop / n * 1e-6:7.1f} TFLOP/s   extend {o:9.1f} us {flop / o * 1e-6:7.1f} TFLOP/s   "
          f"chunk / extend {n / o:5.2f}   max |chunk - extend| {diff:.1e}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(DEFAULT_SHAPES))
    ap.add_argument("--layouts", default="replicated,shared")
    ap.add_argument("--out", default=None, help="also write the table here")
    ap.add_argument("--limit", type=int, default=240, help="seconds per (layout, shape)")
    ap.add_argument("--case", default=None, help=argparse.SUPPRESS)               # (the child: LAYOUT:BxRxT)
    args = ap.parse_args()
    if args.case:
        layout, shape = args.case.split(":")
        import torch
        print(f"# {torch.cuda.get_device_name()}", flush=True)
        case(layout, *(int(x) for x in shape.split("x")))
        return 0
    # (the parent never opens the GPU: every measurement, and the device's name, comes from a fresh child process)
    lines = [f"# causal attention of T new tokens per request over the paged INT4 cache, {Q_HEADS} query / {KV_HEADS} KV heads, head_dim {HD}, pages of {PAGE} "
             "rows; requests x cached rows (the T new ones included); us per launch (median of 5 rounds of a captured graph of 20 launches, the two "
             "launches alternating); TFLOP/s counts the causal work; replicated: the reference's layout read one copy per KV head, shared: the KV heads once"]
    print(lines[0], flush=True)
    for layout in args.layouts.split(","):
        for shape in args.shapes.split(","):
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", f"{layout}:{shape}"], capture_output=True, text=True,
                                   timeout=args.limit)
            except subprocess.TimeoutExpired:
                print(f"# {layout} {shape}: no result within {args.limit} s: stopping", flush=True)
                return 124
            print(r.stdout, end="", flush=True)
            if r.returncode != 0:
                print(r.stderr[-2000:], f"\n# {layout} {shape}: the child ended with {r.returncode}: stopping", flush=True)
                return r.returncode if r.returncode > 0 else 1
            lines += [ln for ln in r.stdout.splitlines() if ln not in lines]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
