"""Which kernel every Kronecker transform + quantiser launch runs, pinned on the CPU: a table of launch -> fq_debug_kron_route answer.

fq_kron_route (csrc/fq_kron_route.hip) is the one place that decides it; it is host arithmetic, so this needs no GPU. The expected
answers were NOT taken from that function: they were recorded from the library as it stood before the decision was gathered there
(version 120, a cascade of "not mine, ask the next family" through ten launchers), by driving every case below through the C entry
point it belongs to and noting the kernel each call handed to hipLaunchKernel (name with template arguments; the fragment-image
preparation kernels set aside) — the same names a `rocprofv3 --kernel-trace` of the calls shows (profiles/kron_route_refactor.txt,
which also holds grids, block sizes, LDS sizes and output hashes of both libraries). A call the old library refused is recorded as
"-1001" where fq_last_error() asked for a workspace and as "-1000" otherwise.

`python tests/test_kron_route_cpu.py` prints the table for whatever library is loaded (FQHIP_LIB), in the form EXPECTED has; a
library from before fq_debug_kron_route has to be traced instead.

Case ids: "<form> <h|b> <M>x<N> f<flags, hex> [c<n_clips>] [d] [r<rows>] [w<workspace bytes>]"; form k = fq_kron_quant_*, r = fq_rmsnorm_kron_quant_ws_f16,
s = fq_silu_mul_kron_quant_f16, e / E = fq_kron_quant_ex_f16 with post_scale 0.5 (E: and `up`), g = fq_kron_quant_grouped_*; h = f16, b = bf16;
d = with diag; defaults: one clip set, 3 rows, a workspace of 1 GiB.
"""
import ast
import os
import re

import pytest

from tests import edge_tokens
from tests.test_gpu_bounds import OUTPUT_SETS, PAIRS

P, F, T, R16, NC0, Q16, PREPARED, G128 = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40, 0x200
FORMS = {"k": 0, "r": 1, "s": 2, "e": 3, "E": 3, "g": 4}
BIG_WS = 1 << 30

# every pair the GPU files name, and the boundaries the route branches on: M at 64/65, 96/97, 128/129, 160/161, 192/193 at the widths of
# the families that split there; odd M at N = 148; N = 63 and M * N just over 32768 (rejected); M > 256
BOUNDARY = [(64, 128), (65, 128), (96, 128), (97, 128), (128, 128), (129, 128), (64, 64), (65, 64), (96, 64), (97, 64), (128, 64), (129, 64),
            (160, 64), (161, 64), (192, 64), (193, 64), (64, 112), (65, 112), (96, 112), (97, 112), (96, 224), (97, 224), (128, 224), (129, 224),
            (96, 144), (97, 144), (128, 144), (129, 144), (128, 192), (129, 192), (144, 192), (145, 192), (160, 176), (161, 176), (192, 176),
            (193, 176), (127, 148), (96, 148), (97, 148), (129, 148), (64, 63), (256, 130), (128, 256), (129, 256), (257, 2), (172, 64)]
ALL_PAIRS = sorted({mn for fam in list(PAIRS.values()) + list(edge_tokens.PAIRS.values()) for mn in fam} | set(BOUNDARY))
ONE_PER_FAMILY = [(64, 64), (64, 128), (56, 64), (112, 128), (86, 128), (128, 224), (128, 148), (172, 64), (80, 64), (112, 256), (20, 12), (129, 254)]
SETS = OUTPUT_SETS + [T | Q16, F | R16, P | T | Q16 | R16, P | T]   # + transform-only with FQ_QUANT_F16; fake-quant-only is OUTPUT_SETS' F
G128_SETS = [P | G128, P | R16 | G128, F | R16 | G128, P | F | T | R16 | G128, P | Q16 | R16 | G128]


def cases():
    """-> [(id, dict(form, bf16, M, N, flags, n_clips, diag, rows, ws, in2, post_scale))]"""
    out = []

    def add(form, bf, M, N, flags, n_clips=1, diag=False, rows=3, ws=BIG_WS):
        cid = f"{form} {'b' if bf else 'h'} {M}x{N} f{flags:x}" + (f" c{n_clips}" if n_clips != 1 else "") + (" d" if diag else "") + (
            f" r{rows}" if rows != 3 else "") + (f" w{ws}" if ws != BIG_WS else "")
        out.append((cid, dict(form=FORMS[form], bf16=bf, M=M, N=N, flags=flags, n_clips=n_clips, diag=diag, rows=rows, ws=ws, in2=form in "sE",
                              post_scale=0.5 if form in "eE" else 1.0)))

    for bf in (False, True):
        for M, N in ALL_PAIRS:
            for flags in SETS:
                for diag in (False, True):
                    add("k", bf, M, N, flags, diag=diag)
            if (M * N) % 128 == 0:                       # (kron_dispatch refuses the other FQ_GROUP128 launches before it routes)
                for flags in G128_SETS:
                    add("k", bf, M, N, flags)
            for flags in (P, F, P | T, F | T | Q16):
                add("g", bf, M, N, flags)
        for M, N in ONE_PER_FAMILY:
            for flags in SETS:
                for n_clips in ((0, 4) if not flags & (P | F) else (4,)):
                    add("k", bf, M, N, flags, n_clips=n_clips)
            for flags in (P, P | F | T | R16):
                for ws in (0, 1000, 20000):              # absent, too small, enough for 64 x 64's second kernel but not for both images
                    add("k", bf, M, N, flags, ws=ws)
                add("k", bf, M, N, flags | PREPARED)
                add("k", bf, M, N, flags | PREPARED, ws=20000)
    for M, N in ALL_PAIRS:
        for flags in (P, P | T, T):
            add("r", False, M, N, flags, n_clips=2)
        for flags in (P, P | Q16 | R16, P | F | T | R16, F):
            for rows in (3, 64, 65):
                add("s", False, M, N, flags, rows=rows)
            add("E", False, M, N, flags)
        for flags in (P, P | Q16 | R16, T, P | T | Q16 | R16, P | T):
            add("e", False, M, N, flags)
        add("s", False, M, N, P, ws=0)
        add("e", False, M, N, P, ws=1000)
    return out


def route(lib_mod, c):
    return lib_mod.kron_route(c["M"], c["N"], c["flags"], rows=c["rows"], bf16=c["bf16"], form=c["form"], n_clips=c["n_clips"], diag=c["diag"],
                              in2=c["in2"], post_scale=c["post_scale"], workspace_bytes=c["ws"])


def _expected():
    """EXPECTED (answer -> its case ids, in tests/golden/kron_route_v120.txt: one answer per line, then its ids separated by ';')"""
    table = {}
    with open(os.path.join(os.path.dirname(__file__), "golden", "kron_route_v120.txt")) as f:
        for line in f:
            answer, ids = line.rstrip("\n").split("\t")
            for cid in ids.split(";"):
                table[cid] = answer
    return table


def test_every_case_routes_as_the_cascade_did():
    from flatquant_amd import _lib
    want, all_cases = _expected(), cases()
    assert set(want) == {cid for cid, _ in all_cases}, "the recorded table and cases() have drifted apart"
    wrong = [(cid, want[cid], got) for cid, c in all_cases for got in [route(_lib, c)] if got != want[cid]]
    assert not wrong, (len(wrong), wrong[:10])


def test_the_rejections_the_issue_names():
    from flatquant_amd import _lib
    for M, N in ((64, 63), (256, 130), (257, 2)):
        for bf in (False, True):
            assert _lib.kron_route(M, N, P, bf16=bf) == "-1000", (M, N)
    assert _lib.kron_route(112, 128, P, workspace_bytes=0) == "-1001"
    assert _lib.kron_route(64, 64, P, workspace_bytes=0).startswith("fq_kron64_kernel<1,")      # (the workspace is optional at 64 x 64)


def test_every_budgeted_kernel_of_these_families_is_reached():
    """tests/test_host_cpu.py holds occupancy budgets by kernel name: each of them that belongs to a family fq_kron_route picks from
    is the answer of at least one case above (an instantiation no launch can select has no business in the budget, or in the library)"""
    src = open(os.path.join(os.path.dirname(__file__), "test_host_cpu.py")).read()
    body = src[src.index("    budget = {"):]
    budget = ast.literal_eval(re.sub(r"^\s*budget = ", "", body[:body.index("\n    }") + 6].strip()))
    families = ("fq_kron64_kernel", "fq_kron_wave_kernel", "fq_kron_tiles_kernel", "fq_kron_trio_kernel", "fq_kron_duo_kernel",
                "fq_kron_tall_kernel", "fq_kron_fast_kernel", "fq_kron_general_kernel")
    named = {k for k in budget if k.split("<")[0] in families}
    assert len(named) >= 30
    assert not named - set(_expected().values()), sorted(named - set(_expected().values()))


@pytest.mark.parametrize("labels,name", [(PAIRS, "tests/test_gpu_bounds.py"), (edge_tokens.PAIRS, "tests/edge_tokens.py")])
def test_the_family_labels_of_the_gpu_files(labels, name):
    for fam, pairs in labels.items():
        for M, N in pairs:
            assert edge_tokens.packed_family(M, N) == fam, (name, fam, M, N)


if __name__ == "__main__":
    from flatquant_amd import _lib
    by_answer = {}
    for cid, c in cases():
        by_answer.setdefault(route(_lib, c), []).append(cid)
    for answer in sorted(by_answer):
        print(answer + "\t" + ";".join(by_answer[answer]))
