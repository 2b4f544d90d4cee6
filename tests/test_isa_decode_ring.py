"""The hot loop of every `decode_mfma_kernel` instance keeps K/V tiles in flight, as compiled.

The matrix-core paged decode holds a ring of three tiles in registers.  As first compiled it never had more than one in
flight: the page id of every tile came from a `global_load_dword` followed by `s_waitcnt vmcnt(0)` and `v_readfirstlane_b32`
(vector loads return in order, so the wait for the id retired every K/V load issued before it), and because every tile load
of the loop was conditional the compiler waited `vmcnt(7) ... vmcnt(0)` for a tile it had just requested.  No result changed
and no test could see it.  `scripts/check_decode_ring.py` reads the waits of the compiled loop; here it runs on
paged_decode_gqa.hip compiled with the library's flags, together with the compiler's resource remarks (no scratch).
"""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mojo_opset_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def _hipcc():
    return shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


@pytest.mark.skipif(_hipcc() is None, reason="no hipcc")
def test_the_compiled_ring_keeps_tiles_in_flight_and_uses_no_scratch(tmp_path):
    import check_decode_ring as chk

    out = str(tmp_path / "paged_decode_gqa.s")
    cmd = [_hipcc(), "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-fno-gpu-rdc", "-ffp-contract=on", "-w",
           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
           "-o", out, os.path.join(CSRC, "paged_decode_gqa.hip")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(out) as f:
        stats, report = chk.check_listing(f.readlines())
    # fp16 / bf16 x head_dim 64 / 128 x nt / cached x (split, fused, paired) + the windowed (split, fused): 40 instances
    assert len(stats) == 40, sorted(stats)
    assert not report, report[:5]
    for name, s in stats.items():
        # the loop really is the ring: three tiles a round, eight loads and sixteen MFMAs each (and the parser still sees them)
        assert s["mfma"] == 48 and s["loads"] == 24 and s["min_vmcnt"] is not None and s["min_vmcnt"] >= chk.STEP_LOADS, (name, s)
        # the loop around it is the window hand-over: one id-window request, and no wait that reaches into the ring
        assert s["outer_loads"] == 1 and (s["outer_min_vmcnt"] is None or s["outer_min_vmcnt"] >= chk.STEP_LOADS), (name, s)
    res, bad = chk.check_resources(r.stderr)
    assert set(res) == set(stats)
    assert not bad, bad
    for name, v in res.items():
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0, (name, v)
        if "Li0ELb" not in name:                            # the 512-thread forms (fused, paired): two waves per SIMD
            assert v["occupancy"] >= 2, (name, v)


def test_the_checker_sees_the_single_buffer_it_was_written_for():
    """A reduced listing of the loop top as first compiled: the id load and its drain, eight tile loads, the conservative join."""
    import check_decode_ring as chk

    tile = "".join(f"\tglobal_load_dwordx4 v[{100 + 4 * i}:{103 + 4 * i}], v[84:85], off nt\n" for i in range(8))
    joins = "".join(f"\ts_waitcnt vmcnt({n})\n\tv_mfma_f32_16x16x32_bf16 v[0:3], v[{40 + 4 * n}:{43 + 4 * n}], v[20:23], v[0:3]\n"
                    for n in range(7, -1, -1))
    head = "_ZN4mojo18decode_mfma_kernelIDF16bLi4ELb1ELi2ELb0EEEvNS_10DecodeArgsEi:\n\ts_load_dwordx4 s[0:3], s[4:5], 0x0\n.LBB0_9:\n"
    tail = "\ts_cbranch_scc1 .LBB0_9\n\ts_endpgm\n.Lfunc_end0:\n"
    id_fetch = "\tglobal_load_dword v2, v[6:7], off\n\ts_waitcnt vmcnt(0)\n\tv_readfirstlane_b32 s8, v2\n"
    bad = head + id_fetch + tile + joins + tail
    stats, report = chk.check_listing(bad.splitlines(keepends=True))
    assert [{k: s[k] for k in ("mfma", "loads", "min_vmcnt")} for s in stats.values()] == [{"mfma": 8, "loads": 9, "min_vmcnt": 0}]
    assert sum("feeds" in r for r in report) == 1, report
    assert sum("outstanding" in r for r in report) == 9, report          # the drain and vmcnt(7) ... vmcnt(0)
    # the same loop with the id read from a register and counted waits: nothing to report
    counted = joins
    for n in range(7, -1, -1):
        counted = counted.replace(f"vmcnt({n})\n", f"vmcnt({n + 16})\n")
    good = head + "\tv_readlane_b32 s8, v2, s9\n" + tile + counted + tail
    stats, report = chk.check_listing(good.splitlines(keepends=True))
    assert [{k: s[k] for k in ("mfma", "loads", "min_vmcnt")} for s in stats.values()] == [{"mfma": 8, "loads": 8, "min_vmcnt": 16}]
    assert not report, report
    # the window hand-over in the loop around it, as compiled with the copy behind the refill: the copy out of a third register
    # waits for vmcnt(0).  The block lies behind a block of no loop, as the compiler lays it out
    inner = ".LBB0_9:\n\tv_readlane_b32 s8, v2, s9\n" + tile + counted + "\ts_cbranch_scc1 .LBB0_9\n"
    handover = ("\ts_cbranch_scc0 .LBB0_20\n\ts_branch .LBB0_30\n.LBB0_12:\n\ts_waitcnt vmcnt(0)\n\ts_endpgm\n"
                ".LBB0_20:\n\tglobal_load_dword v116, v[116:117], off\n\tv_mov_b32_e32 v200, v115\n{wait}\tv_mov_b32_e32 v115, v116\n"
                "\ts_branch .LBB0_8\n.LBB0_30:\n")
    pre = head.replace(".LBB0_9:\n", ".LBB0_8:\n")
    for wait, want in (("\ts_waitcnt vmcnt(0)\n", 1), ("", 0), ("\ts_waitcnt vmcnt(24)\n", 0)):
        text = pre + inner + handover.format(wait=wait) + "\ts_endpgm\n.Lfunc_end0:\n"
        stats, report = chk.check_listing(text.splitlines(keepends=True))
        (st,) = stats.values()
        assert st["mfma"] == 8 and st["loads"] == 8 and st["outer_loads"] == 1, st
        assert len(report) == want and all("enclosing loop" in r for r in report), (wait, report)
    # a kernel of another name is not looked at; scratch is read from the remarks
    assert chk.check_listing(bad.replace("decode_mfma_kernel", "other_kernel").splitlines(keepends=True)) == ({}, [])
    remarks = ("x.h:59:1: remark: Function Name: _ZN4mojo18decode_mfma_kernelIDF16bLi4ELb1ELi2ELb0EEEvNS_10DecodeArgsEi [-Rpass-analysis=kernel-resource-usage]\n"
               "x.h:59:1: remark:     VGPRs: 256 [-Rpass-analysis=kernel-resource-usage]\n"
               "x.h:59:1: remark:     ScratchSize [bytes/lane]: 8 [-Rpass-analysis=kernel-resource-usage]\n"
               "x.h:59:1: remark:     Occupancy [waves/SIMD]: 2 [-Rpass-analysis=kernel-resource-usage]\n"
               "x.h:59:1: remark:     VGPRs Spill: 1 [-Rpass-analysis=kernel-resource-usage]\n")
    res, bad = chk.check_resources(remarks)
    assert list(res.values()) == [{"vgprs": 256, "scratch": 8, "occupancy": 2, "vgpr_spill": 1}] and len(bad) == 1
