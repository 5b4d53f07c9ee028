#!/usr/bin/env python3
"""Print the one-line JSON records of bench.py as a small table: tools/show_bench.py a.json b.json ..."""
import json
import sys

for path in sys.argv[1:]:
    try:
        d = json.load(open(path))
    except Exception as e:  # noqa: BLE001
        print(path, "no json:", e)
        continue
    head = f"{path}: {d['value']:.3e} Melem/s, {d['ms_per_step'] * 1e3:.1f} us/step, n_gpus {d['n_gpus']}"
    r = d.get("roofline")
    if r is None:                      # a plain bench.py line: the roofline comes with --full
        print(head)
        continue
    print(f"{head} | dominant: {r['kernel']} {r['launch_us']:.1f} us frac {r['frac']:.3f} | step frac {r.get('step', {}).get('frac')}")
    for k in r.get("kernels", []):
        print(f"     {k['kernel']:58s} {k['launch_us']:8.1f} us  frac {k['frac']:.3f}")
