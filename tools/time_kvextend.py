#!/usr/bin/env python3
"""Causal attention of T new tokens per request over the paged KV cache (ops.kv_batch_extend -> fq_kv_batch_extend) against the decode launch
(ops.kv_batch_decode) of the same cache: one decode launch, and T sequential decode launches (what a T-token verify step costs without the
extend launch). Llama-3-8B heads (32 query / 8 KV, head_dim 128), 2048 cached tokens per request including the step's T.
    tools/time_kvextend.py [--layouts replicated,shared,fp16] [--batches 1,4,16,64] [--tokens 1,2,4,8,16]
Each figure is the median over rounds of a captured graph of STEPS launches (the per-call Python cost is not in it); the three forms are
measured alternately in the same process, round by round."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from flatquant_amd import ops  # noqa: E402

Q_HEADS, KV_HEADS, HD, SEQ = 32, 8, 128, 2048


def graph_of(fn, steps):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()                                       # (eager first: the split workspaces exist before the capture)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        for _ in range(steps):
            fn()
    return g


def timed(g, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / steps


def case(layout, bsz, T, rounds=7, steps=20):
    g = torch.Generator(device="cuda").manual_seed(0)
    fp16 = layout == "fp16"
    cache_heads, copies = (KV_HEADS, 1) if layout == "shared" else (Q_HEADS, Q_HEADS // KV_HEADS)
    page = SEQ
    if fp16:
        data = torch.randn(bsz, 1, 2, cache_heads, page, HD, generator=g, device="cuda").half()
    else:
        data = torch.randint(0, 256, (bsz, 1, 2, cache_heads, page, HD // 2), generator=g, device="cuda", dtype=torch.uint8)
    par = (torch.rand(bsz, 1, 2, cache_heads, page, 2, generator=g, device="cuda") * 0.2 + 0.05).half()
    indptr = torch.arange(bsz + 1, device="cuda", dtype=torch.int32)
    indices = torch.randperm(bsz, generator=g, device="cuda").to(torch.int32)
    last = torch.full((bsz,), SEQ, device="cuda", dtype=torch.int32)
    q = torch.randn(bsz, T, Q_HEADS, HD, generator=g, device="cuda").half()
    q1 = q[:, 0].contiguous()
    ext = lambda: ops.kv_batch_extend(q, data, par, indptr, indices, last, 0, seq_hint=SEQ, kv_copies=copies)
    dec = lambda: ops.kv_batch_decode(q1, data, par, indptr, indices, last, 0, seq_hint=SEQ, kv_copies=copies)

    def seq_dec():
        for _ in range(T):
            dec()
    graphs = [graph_of(ext, steps), graph_of(dec, steps), graph_of(seq_dec, steps)]
    us = [[], [], []]
    for _ in range(rounds):
        for i, gr in enumerate(graphs):
            us[i].append(timed(gr, steps))
    e, d, s = (statistics.median(u) for u in us)
    print(f"{layout:<10s} bsz={bsz:<3d} T={T:<3d} extend {e:8.1f} us   one decode {d:8.1f} us   {T} decodes {s:8.1f} us   "
          f"extend / {T} decodes {e / s:5.2f}   extend / one decode {e / d:5.2f}", flush=True)
    del graphs
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layouts", default="replicated,shared,fp16")
    ap.add_argument("--batches", default="1,4,16,64")
    ap.add_argument("--tokens", default="1,2,4,8,16")
    args = ap.parse_args()
    print(f"# {torch.cuda.get_device_name()}; {Q_HEADS} query / {KV_HEADS} KV heads, head_dim {HD}, {SEQ} cached tokens per request (page {SEQ}); "
          "replicated: the reference's layout read one copy per KV head; shared: the KV heads once; fp16: fp16 pages, replicated, one copy read")
    with torch.no_grad():
        for layout in args.layouts.split(","):
            for bsz in (int(v) for v in args.batches.split(",")):
                for T in (int(v) for v in args.tokens.split(",")):
                    case(layout, bsz, T)


if __name__ == "__main__":
    main()
