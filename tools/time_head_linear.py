#!/usr/bin/env python3
"""The fused o_proj launch (fq_block_linear_f16: head transform 128 x 32 + quantiser + the 4096 x 4096 Linear4bit) against the two launches it
replaces (fq_block_quant_f16 -> fq_int4_skinny_linear_f16), M = 1 .. 16 tokens: us per call from a captured HIP graph of REPS calls each (what a
captured decode step sees), the weights rotated over enough images (~400 MB) that they stream from HBM as in a real model. The two forms are
timed alternately, REPEATS times each; the table gives the median of each and the spread (max - min) of the two-launch time, which is what
deploy.nn.linear.FUSED_HEAD_ROWS is set by: the largest M up to which the fused launch wins by more than that spread."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flatquant_amd import ops  # noqa: E402
from flatquant_amd._lib import FQ_NO_CLAMP0, FQ_OUT_PACKED  # noqa: E402

REPS = int(os.environ.get("REPS", "40"))
REPEATS = int(os.environ.get("REPEATS", "3"))
N, K, R, C = 4096, 4096, 128, 32


def graph_time(fn, warm):
    """us per call: the median of seven replays of a graph of REPS calls"""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for i in range(warm):
            fn(i)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for i in range(REPS):
                fn(i)
        for _ in range(3):
            g.replay()
        torch.cuda.synchronize()
        ts = []
        for _ in range(7):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3 / REPS)
    return sorted(ts)[len(ts) // 2]


def main():
    gen = torch.Generator(device="cuda").manual_seed(0)
    nb = max(6, int(400e6 // (N * K // 2)))
    imgs = [ops.int4_to_frag(torch.randint(0, 256, (N, K // 2), generator=gen, device="cuda", dtype=torch.uint8)) for _ in range(nb)]
    wss = [torch.rand(N, generator=gen, device="cuda").half() * 0.01 for _ in range(nb)]      # (a layer's own scales: cold, like its weights)
    P = (torch.randn(C, C, generator=gen, device="cuda") / C ** 0.5).half()
    sig = (0.98, 0.98)
    print(f"o_proj pair, {N} x {K} INT4 weights rotated over {nb} images, graph of {REPS} calls, {REPEATS} alternating repeats; us per call")
    print(" M | two launches: median   min   max  spread | fused: median   min   max | gain  | fused wins by more than the spread | exact")
    best = 0
    for M in range(1, 17):
        x = torch.randn(M, R, C, generator=gen, device="cuda").half()

        def two(i):
            o = ops.block_quant(x, P, [sig], FQ_OUT_PACKED | FQ_NO_CLAMP0, transpose_out=True)
            return ops.int4_skinny_linear(o.q[0].reshape(M, K // 2), o.scale[0], imgs[i % nb], wss[i % nb], None, N)

        def one(i):
            return ops.block_linear(x, P, sig, imgs[i % nb], wss[i % nb], None, N, flags=FQ_NO_CLAMP0)

        ok = torch.equal(two(0), one(0))
        t2, t1 = [], []
        for _ in range(REPEATS):
            t2.append(graph_time(two, nb))
            t1.append(graph_time(one, nb))
        t2.sort(), t1.sort()
        m2, m1, spread = t2[len(t2) // 2], t1[len(t1) // 2], t2[-1] - t2[0]
        wins = m2 - m1 > spread
        if wins and best == M - 1:
            best = M
        print(f"{M:2d} | {m2:20.2f} {t2[0]:5.2f} {t2[-1]:5.2f} {spread:7.2f} | {m1:13.2f} {t1[0]:5.2f} {t1[-1]:5.2f} | {m2 - m1:5.2f} | {'yes' if wins else 'no':>34s} | {ok}",
              flush=True)
    print(f"largest M up to which the fused launch wins at every M by more than the two-launch spread: {best}")


if __name__ == "__main__":
    main()
