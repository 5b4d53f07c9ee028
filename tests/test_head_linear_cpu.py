"""fq_block_linear_f16 without a GPU: the symbol and its declaration, the argument checks of the C entry (they return before any HIP call, the
pointers are never dereferenced), the compiler's resource report of the new kernel and of the kernels it must not move, the routing constant."""
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_declared_with_fourteen_arguments():
    from flatquant_amd import _lib
    assert "fq_block_linear_f16" in _lib.SYMBOLS
    restype, argtypes = _lib.SYMBOLS["fq_block_linear_f16"]
    assert restype is ctypes.c_int and len(argtypes) == 14
    assert argtypes[2] is ctypes.c_int64 and argtypes[5] is ctypes.c_float and argtypes[6] is ctypes.c_float
    header = open(os.path.join(ROOT, "include", "fqhip.h")).read()
    m = re.search(r"\bint\s+fq_block_linear_f16\s*\(([^)]*)\)\s*;", header)
    assert m, "not declared in include/fqhip.h"
    assert len(m.group(1).split(",")) == 14
    assert hasattr(_lib.lib, "fq_block_linear_f16")


def test_argument_checks_return_before_any_launch():
    from flatquant_amd._lib import FQ_EINVAL, FQ_EUNSUPPORTED, FQ_NO_CLAMP0, FQ_OUT_PACKED, FQ_ROUND_Y_F16, lib
    vp = 0x1000

    def call(x=vp, P=vp, M=4, R=128, C=32, smax=1.0, smin=1.0, flags=FQ_NO_CLAMP0, img=vp, ws=vp, bias=None, N=4096, y=vp):
        return lib.fq_block_linear_f16(x, P, M, R, C, ctypes.c_float(smax), ctypes.c_float(smin), flags, img, ws, bias, N, y, None)
    for name in ("x", "P", "img", "ws", "y"):
        assert call(**{name: None}) == FQ_EINVAL, name
        assert b"NULL" in lib.fq_last_error(), name
    for name in ("x", "P", "img"):
        assert call(**{name: 0x1008}) == FQ_EINVAL, name
        assert b"16-byte aligned" in lib.fq_last_error(), name
    for name in ("ws", "bias", "y"):
        assert call(**{name: 0x1001}) == FQ_EINVAL, name
        assert b"2-byte aligned" in lib.fq_last_error(), name
    assert call(M=0) == FQ_EINVAL and b"M=0" in lib.fq_last_error()
    assert call(M=-1) == FQ_EINVAL and call(N=0) == FQ_EINVAL and call(N=-32) == FQ_EINVAL
    for bad in (FQ_OUT_PACKED, FQ_ROUND_Y_F16, FQ_NO_CLAMP0 | FQ_ROUND_Y_F16, 0x40000000):
        assert call(flags=bad) == FQ_EINVAL, hex(bad)
        assert b"flag" in lib.fq_last_error()
    assert call(smax=0.0) == FQ_EINVAL and call(smin=-1.0) == FQ_EINVAL
    assert call(M=17) == FQ_EUNSUPPORTED and b"M=17" in lib.fq_last_error()
    assert call(R=64, C=64) == FQ_EUNSUPPORTED and b"C=64" in lib.fq_last_error()          # C = 64
    assert call(R=64, C=32) == FQ_EUNSUPPORTED and call(R=128, C=16) == FQ_EUNSUPPORTED   # R C != 4096
    assert call(N=48) == FQ_EUNSUPPORTED and b"N=48" in lib.fq_last_error()
    assert call(N=16) == FQ_EUNSUPPORTED


def _sgprs(file, mangled_part):
    """TotalSGPRs of the kernels of build/<file>.res whose mangled name contains `mangled_part` (tools/kernel_resources.py does not keep them)"""
    out, cur = [], None
    for line in open(os.path.join(ROOT, "flatquant_amd", "csrc", "build", file + ".res"), errors="replace"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
        m = re.search(r"remark:\s+TotalSGPRs: (\d+)", line)
        if m and cur is not None and mangled_part in cur:
            out.append(int(m.group(1)))
    return out


def test_resource_reports_of_the_new_kernel_and_of_its_model():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import parse
    res = parse()
    new = {k: r for k, r in res.items() if r["file"] == "fq_block_linear"}
    if not new:
        pytest.skip("no build/fq_block_linear.res next to the sources (library built elsewhere)")
    assert set(new) == {"fq_block_linear_kernel"}, sorted(new)
    r = new["fq_block_linear_kernel"]
    assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, r
    assert r["occupancy"] >= 2 and r["lds"] == 0, r          # eight waves per workgroup: two per SIMD; the LDS is dynamic (<= 43.6 KB)
    # fq_kron64_linear_kernel<RMS>: the values of the build this kernel was added to — nothing of that file is shared or moved
    parent = {"fq_kron64_linear_kernel<1>": dict(vgpr=209, sgpr=58), "fq_kron64_linear_kernel<0>": dict(vgpr=204, sgpr=58)}
    for name, p in parent.items():
        k = res[name]
        assert k["file"] == "fq_kron64"
        assert (k["vgpr"], k["agpr"], k["occupancy"], k["vgpr_spill"], k["sgpr_spill"], k["scratch"], k["lds"]) == (p["vgpr"], 0, 2, 0, 0, 0, 0), (name, k)
    assert _sgprs("fq_kron64", "fq_kron64_linear_kernelILb1E") == [58] and _sgprs("fq_kron64", "fq_kron64_linear_kernelILb0E") == [58]


def test_routing_constant_and_supported_shapes():
    from flatquant_amd import ops
    from flatquant_amd.deploy.nn import linear
    c = linear.FUSED_HEAD_ROWS
    assert isinstance(c, int) and not isinstance(c, bool) and 0 <= c <= 16, c
    assert ops.block_linear_supported(1, 128, 32, 4096) and ops.block_linear_supported(16, 128, 32, 32) and ops.block_linear_supported(8, 128, 32, 40960)
    assert not ops.block_linear_supported(17, 128, 32, 4096) and not ops.block_linear_supported(0, 128, 32, 4096)
    assert not ops.block_linear_supported(4, 64, 64, 4096) and not ops.block_linear_supported(4, 64, 32, 4096)
    assert not ops.block_linear_supported(4, 128, 32, 48) and not ops.block_linear_supported(4, 128, 32, 0)


def test_fuse_reports_o_proj_only_when_asked():
    """the default report is unchanged (existing tests compare it for equality); with the flag a pair of another form is refused"""
    import torch

    import flatquant_amd.deploy as deploy
    m = torch.nn.Module()
    assert deploy.fuse(m) == {"transform_groups": 0, "linear_groups": 0, "down_proj": 0}
    assert deploy.fuse(m, o_proj=True) == {"transform_groups": 0, "linear_groups": 0, "down_proj": 0, "o_proj": 0}
    m.o_proj_trans = deploy.nn.OnlineTrans(32, trans="matmul", decompose=False)
    m.o_proj = torch.nn.Sequential(deploy.nn.Quantizer(lac=True), deploy.nn.Linear4bit(4096, 64))
    assert deploy.fuse(m) == {"transform_groups": 0, "linear_groups": 0, "down_proj": 0} and "_group" not in m.o_proj_trans.__dict__
    assert deploy.fuse(m, o_proj=True)["o_proj"] == 1
    assert m.o_proj_trans.__dict__["_group"] is m.o_proj[1].__dict__["_group"]
    deploy.unfuse(m)
    assert "_group" not in m.o_proj_trans.__dict__ and "_group" not in m.o_proj[1].__dict__
    bad = torch.nn.Module()
    bad.o_proj_trans = deploy.nn.OnlineTrans(4096, trans="matmul", decompose=True)
    bad.o_proj = torch.nn.Sequential(deploy.nn.Quantizer(lac=True), deploy.nn.Linear4bit(4096, 64))
    with pytest.raises(RuntimeError):
        deploy.fuse(bad, o_proj=True)
