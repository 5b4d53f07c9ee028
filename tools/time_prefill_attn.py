#!/usr/bin/env python3
"""The prompt attention launch (ops.prefill_attention -> fq_prefill_attention_f16) against torch's scaled_dot_product_attention(is_causal=True)
on the same tensors: Llama-3-8B's prompt shapes (32 query / 8 KV heads, head_dim 128), 8 x 2048 and 1 x 8192 tokens.
    tools/time_prefill_attn.py [--shapes 8x2048,1x8192] [--out profiles/prefill_attn.txt] [--limit 240]
Every shape is measured in a child process of its own under a time limit (--limit seconds); a child that fails or runs out of time ends the run.
Figures: the median over rounds of event-timed batches of launches after a warm-up, the inputs rotating through as many sets as it takes to
exceed twice the 256 MB Infinity Cache (no launch finds its K / V where the previous one left them); TFLOP/s counts the causal half
(2 b H s^2 d). torch gets the KV heads expanded beforehand (not timed) and [b, H, s, d] views of the same memory; with --trans the launch
also forms q . q_trans itself, torch is given the product (its matmul is not timed either)."""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q_HEADS, KV_HEADS, HD = 32, 8, 128
CACHE_BYTES = 256 << 20


def timed(fn, sets, launches):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(launches):
        fn(sets[i % len(sets)])
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / launches


def case(bsz, seq, trans, rounds=7, launches=10):
    import torch
    sys.path.insert(0, ROOT)
    from flatquant_amd import ops
    g = torch.Generator(device="cuda").manual_seed(0)
    one = 2 * (2 * bsz * seq * Q_HEADS * HD + 2 * bsz * seq * KV_HEADS * HD)      # q, o, k, v of a set in bytes
    nsets = max(2, -(-2 * CACHE_BYTES // one))
    qt = torch.linalg.qr(torch.randn(HD, HD, generator=g, device="cuda"))[0].half().contiguous() if trans else None
    sets = []
    for _ in range(nsets):
        q = (torch.randn(bsz, seq, Q_HEADS, HD, generator=g, device="cuda") * 0.5).half()
        k = (torch.randn(bsz, seq, KV_HEADS, HD, generator=g, device="cuda") * 1.5).half()
        v = torch.randn(bsz, seq, KV_HEADS, HD, generator=g, device="cuda").half()
        qq = q if qt is None else torch.matmul(q, qt)
        grp = Q_HEADS // KV_HEADS
        sets.append({"q": q, "k": k, "v": v, "tq": qq.transpose(1, 2), "tk": k.repeat_interleave(grp, dim=2).transpose(1, 2),
                     "tv": v.repeat_interleave(grp, dim=2).transpose(1, 2)})
    ours = lambda s: ops.prefill_attention(s["q"], s["k"], s["v"], qt)
    sdpa = lambda s: torch.nn.functional.scaled_dot_product_attention(s["tq"], s["tk"], s["tv"], is_causal=True)
    with torch.no_grad():
        o = ours(sets[0])
        try:
            ref = sdpa(sets[0]).transpose(1, 2)
            diff = (o.float() - ref.float()).abs().max().item()
        except Exception as e:                                                     # (a build without an fp16 causal kernel for this shape)
            print(f"# torch SDPA failed: {type(e).__name__}: {e}", flush=True)
            sdpa, diff = None, float("nan")
        us = {"ours": [], "torch": []}
        for name, fn in (("ours", ours), ("torch", sdpa)):
            if fn is not None:
                timed(fn, sets, 2 * nsets)                                         # warm-up
        for _ in range(rounds):                                                    # alternately, round by round
            for name, fn in (("ours", ours), ("torch", sdpa)):
                if fn is not None:
                    us[name].append(timed(fn, sets, launches))
    flop = 2.0 * bsz * Q_HEADS * seq * seq * HD
    mine = statistics.median(us["ours"])
    line = f"{bsz:>3d} x {seq:<5d} q_trans={'yes' if trans else 'no ':<3s} {nsets:>2d} sets  ours {mine:9.1f} us {flop / mine * 1e-6:7.1f} TFLOP/s"
    if us["torch"]:
        th = statistics.median(us["torch"])
        line += f"   torch SDPA {th:9.1f} us {flop / th * 1e-6:7.1f} TFLOP/s   ours / torch {mine / th:5.2f}   max |ours - torch| {diff:.2e}"
    print(line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="8x2048,1x8192")
    ap.add_argument("--out", default=None, help="also write the table here")
    ap.add_argument("--limit", type=int, default=240, help="seconds per shape")
    ap.add_argument("--case", default=None, help=argparse.SUPPRESS)               # (the child: BxS[t])
    args = ap.parse_args()
    if args.case:
        trans = args.case.endswith("t")
        b, s = (int(x) for x in args.case.rstrip("t").split("x"))
        import torch
        print(f"# {torch.cuda.get_device_name()}", flush=True)
        case(b, s, trans)
        return 0
    # (the parent never opens the GPU: every measurement, and the device's name, comes from a fresh child process)
    lines = [f"# causal prompt attention, {Q_HEADS} query / {KV_HEADS} KV heads, head_dim {HD}, fp16; us per launch (median of 7 rounds of 10 event-timed "
             "launches, inputs rotating through sets larger than twice the Infinity Cache); TFLOP/s counts the causal half"]
    print(lines[0], flush=True)
    for shape in args.shapes.split(","):
        for suffix in ("", "t"):
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", shape + suffix], capture_output=True, text=True, timeout=args.limit)
            except subprocess.TimeoutExpired:
                print(f"# {shape}{suffix}: no result within {args.limit} s: stopping", flush=True)
                return 124
            print(r.stdout, end="", flush=True)
            if r.returncode != 0:
                print(r.stderr[-2000:], f"\n# {shape}{suffix}: the child ended with {r.returncode}: stopping", flush=True)
                return r.returncode if r.returncode > 0 else 1
            lines += [ln for ln in r.stdout.splitlines() if ln not in lines]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
