"""CPU checks of the C-ABI surface of the point-sample backward (``ptx_point_sample_bwd``,
``ptx_point_sample_bwd_workspace_bytes``): declared, bound and exported by both builds, ABI still 13, and every argument check made
on the host before anything is enqueued (the pointers handed in are bogus and never touched)."""
import os
import subprocess

import pytest

from proxytransformation_amd import _abi
from tests.util import header_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTX_EINVAL, PTX_ENOSPACE = -1, -3
NAMES = ("ptx_point_sample_bwd_workspace_bytes", "ptx_point_sample_bwd")


def test_header_declares_and_both_libraries_export_the_backward():
    src = open(os.path.join(ROOT, "include", "proxyt.h")).read()
    protos = header_prototypes()
    assert protos["ptx_point_sample_bwd_workspace_bytes"] == ("size_t", ["int N", "int V", "int H", "int W", "int bilinear"])
    assert protos["ptx_point_sample_bwd"][0] == "int"
    assert "#define PTX_ABI_VERSION 13" in src and _abi.ABI_VERSION == 13
    lib = _abi.lib()
    assert lib.ptx_abi_version() == 13
    for name in NAMES:
        assert name in _abi.SIGNATURES
        getattr(lib, name)
    # the forward's signature is the one the backward mirrors: same image-transform scalars, in the same positions
    fwd, bwd = _abi.SIGNATURES["ptx_point_sample"][1], _abi.SIGNATURES["ptx_point_sample_bwd"][1]
    assert len(fwd) == len(bwd) == 24 and fwd[10:19] == bwd[10:19]
    pkg = os.path.join(ROOT, "proxytransformation_amd")
    for so in ("libproxyt_hip.so", "libproxyt_hip_testhooks.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(pkg, so)], check=True, capture_output=True, text=True).stdout
        exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
        for name in NAMES:
            assert name in exported, (so, name)


def test_workspace_size_follows_the_worst_case_entry_count():
    lib = _abi.lib()
    ws = lib.ptx_point_sample_bwd_workspace_bytes
    near, bil = ws(1000, 50, 120, 120, 0), ws(1000, 50, 120, 120, 1)
    D, E = 50 * 120 * 120, 1000 * 50
    assert near >= 2 * 4 * (D + 1) + 2 * 8 * E and near % 256 == 0
    assert bil - near >= 2 * 8 * 3 * E - 1024                            # four neighbours per (point, view); 256-byte rounding
    assert ws(2000, 50, 120, 120, 0) > near
    for bad in ((0, 50, 120, 120), (1000, 0, 120, 120), (1000, 50, 0, 120), (1000, 50, 120, 0), (-1, 50, 120, 120)):
        assert ws(*bad, 0) == 0
    assert ws(1 << 20, 1 << 10, 8, 8, 1) == 0                            # 2^32 list entries: outside the 32-bit index range
    assert ws(10, 1 << 11, 1 << 10, 1 << 10, 0) == 0                     # 2^31 pixels


GOOD = dict(points=0x1000, N=100, dout=0x2000, valid_num=0x3000, V=4, C=64, H=8, W=8, proj=0x4000, pre=None, sw=1.0, sh=1.0, cw=0.0,
            ch=0.0, flip=0, ori_w=640.0, pad_h=480.0, pad_w=640.0, bilinear=0, dfeats=0x5000, dtype=0, ws=0x6000, ws_bytes=1 << 30)
BAD = {"null_points": dict(points=None), "null_dout": dict(dout=None), "null_valid_num": dict(valid_num=None),
       "null_proj": dict(proj=None), "null_dfeats": dict(dfeats=None), "null_ws": dict(ws=None),
       "N0": dict(N=0), "N_negative": dict(N=-5), "V0": dict(V=0), "C0": dict(C=0), "C513": dict(C=513), "H0": dict(H=0),
       "W0": dict(W=0), "dtype3": dict(dtype=3), "dtype_negative": dict(dtype=-1), "pad_h0": dict(pad_h=0.0),
       "pad_w_negative": dict(pad_w=-640.0), "too_many_pairs": dict(N=1 << 20, V=1 << 10, bilinear=1),
       "too_many_pixels": dict(V=1 << 11, H=1 << 10, W=1 << 10)}


def _call(lib, a):
    return lib.ptx_point_sample_bwd(a["points"], a["N"], a["dout"], a["valid_num"], a["V"], a["C"], a["H"], a["W"], a["proj"],
                                    a["pre"], a["sw"], a["sh"], a["cw"], a["ch"], a["flip"], a["ori_w"], a["pad_h"], a["pad_w"],
                                    a["bilinear"], a["dfeats"], a["dtype"], a["ws"], a["ws_bytes"], None)


@pytest.mark.parametrize("bad", sorted(BAD))
def test_backward_rejects_bad_arguments_before_any_enqueue(bad):
    """Every check is on the host and returns PTX_EINVAL with a message; the pointers are never touched (they are bogus here)."""
    lib = _abi.lib()
    rc = _call(lib, dict(GOOD, **BAD[bad]))
    assert rc == PTX_EINVAL
    msg = lib.ptx_last_error().decode()
    assert msg.startswith("ptx_point_sample_bwd:"), msg


@pytest.mark.parametrize("bilinear", [0, 1])
def test_backward_rejects_a_small_workspace_before_any_enqueue(bilinear):
    lib = _abi.lib()
    need = lib.ptx_point_sample_bwd_workspace_bytes(GOOD["N"], GOOD["V"], GOOD["H"], GOOD["W"], bilinear)
    assert need > 0
    rc = _call(lib, dict(GOOD, bilinear=bilinear, ws_bytes=need - 1))
    assert rc == PTX_ENOSPACE
    msg = lib.ptx_last_error().decode()
    assert msg.startswith("ptx_point_sample_bwd: workspace too small"), msg
