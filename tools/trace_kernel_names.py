#!/usr/bin/env python3
"""Which product kernels a rocprofv3 --kernel-trace run launched, by name WITH template arguments: tools/trace_kernel_names.py <trace dir>
-> launches per kernel instantiation, the __global__ kernels of flatquant_amd/csrc (outside probe/) that never ran, and the rows of the Kronecker
instantiation lists (csrc/fq_kron_route.hpp: the workgroup-per-token and the tiles kernel's) and the decode kernel's (QG, APPEND) pairs that ran or were MISSED.

rocprofv3 leaves most of these names mangled (its demangler does not know _Float16 / __bf16), so the Itanium names are decoded here as far as
kernel template arguments need: <len><name>, I ... E with L<type><value>E literals (i / j / l / m: integers, n = minus; b: bool) and the types
DF16_ (f16) and DF16b (bf16). A name the profiler demangled itself is kept as it printed it, argument list dropped."""
import collections, csv, glob, os, re, sys


def decode(n):
    m = re.match(r"_Z(?:N12_GLOBAL__N_1)?(\d+)", n)
    if not m:
        return None
    L = int(m.group(1))
    name, rest, args = n[m.end():m.end() + L], n[m.end() + L:], []
    if rest.startswith("I"):
        i = 1
        while i < len(rest) and rest[i] != "E":
            if rest.startswith("DF16_", i):
                args.append("f16")
                i += 5
            elif rest.startswith("DF16b", i):
                args.append("bf16")
                i += 5
            elif rest[i] == "L":
                j = rest.index("E", i)
                t, v = rest[i + 1], rest[i + 2:j]
                v = "-" + v[1:] if v.startswith("n") else v
                args.append({"0": "false", "1": "true"}[v] if t == "b" else v)
                i = j + 1
            else:
                return name + "<not decoded: " + rest[i:i + 16] + ">"
    return name + ("<" + ", ".join(args) + ">" if args else "")


def plain(n):
    n = re.sub(r"^void ", "", n.replace("(anonymous namespace)::", "").replace(" [clone .kd]", ""))
    depth = 0
    for i, ch in enumerate(n):
        depth += (ch == "<") - (ch == ">")
        if ch == "(" and depth == 0:
            return n[:i]
    return n


def main(trace_dir):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cnt = collections.Counter()
    for r in csv.DictReader(open(glob.glob(trace_dir + "/**/*kernel_trace.csv", recursive=True)[0])):
        n = r["Kernel_Name"]
        if "fq_" in n:
            cnt[decode(n) or plain(n)] += 1
    print("# launches  kernel<template arguments>")
    for n in sorted(cnt):
        print(f"{cnt[n]:8d}  {n}")
    decl = set()
    for path in glob.glob(os.path.join(root, "flatquant_amd", "csrc", "*.h*")):
        decl.update(re.findall(r"__global__[^;{]*?void\s+(fq_\w+)\s*\(", open(path).read(), re.S))
    ran = {re.split(r"[<(]", n)[0] for n in cnt}
    print(f"\n# {len(decl)} __global__ kernels are declared under flatquant_amd/csrc (outside probe/); never launched in this trace:")
    print("\n".join("   " + n for n in sorted(decl - ran)) or "   (none)")
    print()
    print("\n".join(tables(cnt)))


def route_lists():
    """the instantiation lists of csrc/fq_kron_route.hpp (the source the launch switches are generated from): list name -> rows of ints,
    measurement knobs at their defaults"""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "flatquant_amd", "csrc", "fq_kron_route.hpp")).read()
    knobs = {"true": 1, "false": 0}
    knobs.update({k: int(v) if v.isdigit() else knobs[v] for k, v in re.findall(r"^#define (\w+) (\d+|true|false)\b", src, re.M)})
    lists = {}
    for name, body in re.findall(r"^#define (FQ_KRON_\w+_LIST)\(X\)((?:.*\\\n)*.*)", src, re.M):
        body = re.sub(r"/\*.*?\*/", "", body)
        lists[name] = [tuple(int(t) if t.strip().isdigit() else knobs[t.strip()] for t in row.split(",")) for row in re.findall(r"X\(([^)]*)\)", body)]
    return lists


def tables(cnt):
    """-> lines: every row of the route header's lists with the instantiations of it that ran (or MISSED), and the decode kernel's (QG, APPEND) pairs"""
    args = lambda n: [a.strip() for a in n[n.index("<") + 1:n.rindex(">")].split(",")]
    fast, tiles, dec = collections.defaultdict(set), collections.defaultdict(set), collections.Counter()
    for n in cnt:
        if n.startswith("fq_kron_fast_kernel<") and "not decoded" not in n:
            a = args(n)     # MT, NT, KS1, WAVES, OCC, SILU, CT, NV, T, ...
            fast[(int(a[0]), int(a[1]), int(a[2]), a[5] == "true")].add(f"CT={a[6]}" + (f" W={a[3]}" if a[3] == "8" and a[0:3] == ["4", "4", "8"] else "") + (f" NV={a[7]}" if a[7] != "0" else "") + f" {a[8]}")
        if n.startswith("fq_kron_tiles_kernel<"):
            a = args(n)     # MT, NT, N, GROUPS, LKS, RS, T, H16
            tiles[(int(a[0]), int(a[1]), int(a[2]), int(a[4]))].add(f"{a[6]}{' fp16-quantiser' if a[7] == 'true' else ''}")
        if n.startswith("fq_kv_decode_kernel<"):
            a = args(n)     # HD, NW, UNI, F16, SPLIT, QG, APPEND
            dec[(int(a[5]), a[6] == "true")] += 1
    L = route_lists()
    FQ_F, FQ_FS = [r[:3] for r in L["FQ_KRON_FAST_LIST"]], [r[:3] for r in L["FQ_KRON_FAST_SILU_LIST"]]
    out = ["# FQ_KRON_FAST_LIST rows (MT, NT, KS1): CT = -1 every output set, 1 packed only, 33 packed with the fp16 quantiser (MT >= 3 only)"]
    for r in FQ_F:
        out.append(f"   {r}: " + (", ".join(sorted(fast[r + (False,)])) or "MISSED"))
    out.append("# FQ_KRON_FAST_SILU_LIST rows (SiLU.mul input)")
    for r in FQ_FS:
        out.append(f"   {r}: " + (", ".join(sorted(fast[r + (True,)])) or "MISSED"))
    other = sorted(k for k in fast if k[:3] not in FQ_F)
    out.append("# fq_kron_fast_kernel outside both lists: " + (", ".join(f"{k}: {sorted(fast[k])}" for k in other) or "none ran"))
    out.append("# FQ_KRON_TILES_LIST rows (MT, NT, N, LKS)")
    for r in L["FQ_KRON_TILES_LIST"]:
        out.append(f"   {(r[0], r[1], r[2], r[4])}: " + (", ".join(sorted(tiles[(r[0], r[1], r[2], r[4])])) or "MISSED"))
    out.append("# FQ_KRON_TILES64_LIST rows (MT, LKS) at N = 64")
    for mt, lks, _ in L["FQ_KRON_TILES64_LIST"]:
        out.append(f"   ({mt}, {lks}): " + (", ".join(sorted(tiles[(mt, 2, 64, lks)])) or "MISSED"))
    out.append("# fq_kv_decode_kernel (QG, APPEND) -> instantiations that ran: " + ", ".join(f"{k}: {v}" for k, v in sorted(dec.items())))
    return out


if __name__ == "__main__":
    main(sys.argv[1])
