"""Route table of the dense and 8-bit GEMM entry points: for every case the kernel forms one call launches
(`mojo_hip_launch_history`) and the workspace its `*_workspace_bytes` query asks for, against tests/golden/gemm_routes.json.

The table pins the route decisions — which kernel, which fused form, whether K is split — over rows from one token to a
prefill chunk, both weight layouts and the shapes where every route and its fallbacks appear, so that host-side planner
changes that should not move a route are checked on the hardware.  Routes do not depend on the values: floating-point and
8-bit operands are uninitialised; index inputs (block tables, context lengths) are valid.

    PYTHONPATH=. python tests/test_hip_gemm_routes.py [op ...]   # rewrite the table (or only the named sections) from the
                                                                 # library in use: a deliberate route change, or a new section
                                                                 # recorded from the library BEFORE the change it is to pin
"""
import json
import os
import sys

import pytest
import torch

from hip_utils import DEV, launches_of, switch_env
from mojo_opset_amd.backends.hip import lib as L
from mojo_opset_amd.backends.hip.operators.gemm import (dense_gemm, dense_gemm_residual_rmsnorm, dense_gemm_swiglu,
                                                        qkv_rope_store)

pytestmark = pytest.mark.gpu

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_routes.json")
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32


def _tensor(shape, dtype):
    """An operand whose values do not matter to the route."""
    return torch.empty(shape, dtype=dtype, device=DEV)


def _weight(k, n, kn, dtype):
    return _tensor((k, n) if kn else (n, k), dtype)


# Each generator yields (name, run, workspace): run() makes the call and returns its outputs, workspace() the query's bytes.

def gemm_cases():
    def case(m, k, n, kn, bias, dtype):
        def run():
            return dense_gemm(_tensor((m, k), dtype), _weight(k, n, kn, dtype), _tensor((n,), dtype) if bias else None, kn)
        return f"{str(dtype)[6:]}:{m}x{k}x{n}:{'KN' if kn else 'NK'}{':bias' if bias else ''}", run, \
            lambda: L.load().mojo_hip_gemm_workspace_bytes(m, k, n)

    for k, n in ((4096, 4096), (4096, 14336), (14336, 4096), (8192, 1024), (1024, 8192), (192, 576)):
        for kn in (False, True):
            for m in (1, 8, 16, 33, 64, 65, 100, 128, 129, 256, 512, 1024, 4096):
                yield case(m, k, n, kn, m in (8, 65, 129, 1024), BF16)
    for m in (8, 100, 512):
        for kn in (False, True):
            yield case(m, 4096, 4096, kn, m == 100, F16)
    for m in (8, 256):
        yield case(m, 1024, 1024, False, m == 8, F32)


def resnorm_cases():
    def case(m, k, n, kn, bias, residual):
        def run():
            return dense_gemm_residual_rmsnorm(_tensor((m, k), BF16), _weight(k, n, kn, BF16), _tensor((n,), BF16) if bias else None,
                                               _tensor((m, n), BF16) if residual else None, _tensor((n,), BF16), 1e-6, kn)
        return f"{m}x{k}x{n}:{'KN' if kn else 'NK'}{':bias' if bias else ''}{'' if residual else ':nores'}", run, \
            lambda: L.load().mojo_hip_gemm_residual_rmsnorm_workspace_bytes(m, k, n)

    for k, n in ((4096, 4096), (14336, 4096), (8192, 1024), (1024, 8192)):
        for kn in (False, True):
            for m in (1, 8, 32, 64, 100, 128, 256, 1024):
                yield case(m, k, n, kn, m in (8, 100), m != 32)


def qkv_cases():
    def case(b, k, hq, hkv, d, bias):
        page, pages = 16, 4
        n = (hq + 2 * hkv) * d

        def run():
            kc, vc = _tensor((b * pages, hkv, page, d), BF16), _tensor((b * pages, hkv, page, d), BF16)
            table = torch.arange(b * pages, dtype=torch.int32, device=DEV).reshape(b, pages)
            ctx = (torch.arange(b, dtype=torch.int32, device=DEV) * 7) % (page * pages)
            q = qkv_rope_store(_tensor((b, k), BF16), _weight(k, n, False, BF16), _tensor((n,), BF16) if bias else None,
                               _tensor((b, d), F32), _tensor((b, d), F32), kc, vc, table, ctx, hq, hkv)
            return q, kc, vc
        return f"{b}x{k}:{hq}/{hkv}x{d}{':bias' if bias else ''}", run, \
            lambda: L.load().mojo_hip_qkv_rope_store_workspace_bytes(b, k, n)

    for k, hq, hkv, d in ((4096, 32, 8, 128), (4096, 64, 8, 128), (1024, 8, 2, 64), (4096, 3, 1, 16)):
        for b in (1, 8, 32, 64, 100, 128, 256):
            yield case(b, k, hq, hkv, d, b in (8, 100))


def swiglu_cases():
    def case(m, k, inter):
        def run():
            return dense_gemm_swiglu(_tensor((m, k), BF16), _weight(k, 2 * inter, False, BF16))
        return f"{m}x{k}x{inter}", run, lambda: L.load().mojo_hip_gemm_swiglu_workspace_bytes(m, k, inter)

    for k, inter in ((4096, 14336), (4096, 1024), (1024, 512)):
        for m in (1, 8, 64, 65, 128, 256, 1024, 2048):
            yield case(m, k, inter)


def quant_cases():
    def case(m, k, n, kn, qdtype, odtype):
        def run():
            x, w = _tensor((m, k), qdtype), _weight(k, n, kn, qdtype)
            s_in, s_w = _tensor((m,), F32), _tensor((n,), BF16)
            out = torch.empty(m, n, dtype=odtype, device=DEV)
            lib = L.load()
            ws = torch.empty(lib.mojo_hip_quant_gemm_workspace_bytes(m, k, n), dtype=torch.uint8, device=DEV)
            L.check(lib.mojo_hip_quant_gemm(L.ptr(x), L.ptr(w), L.ptr(s_in), L.ptr(s_w), L.ptr(out), m, k, n, 0 if kn else 1,
                                            L.dtype_code(qdtype), L.dtype_code(odtype), L.ptr(ws), ws.numel(), L.stream_of(x)),
                    "quant_gemm")
            return out
        return f"{str(qdtype)[6:]}>{str(odtype)[6:]}:{m}x{k}x{n}:{'KN' if kn else 'NK'}", run, \
            lambda: L.load().mojo_hip_quant_gemm_workspace_bytes(m, k, n)

    for qdtype in (torch.int8, torch.float8_e4m3fn):
        for k, n in ((4096, 4096), (4096, 14336), (14336, 4096)):
            for kn in (False, True):
                for m in (1, 4, 32, 64, 128, 256, 1024):
                    yield case(m, k, n, kn, qdtype, BF16)
        for m in (1, 64, 1024):
            yield case(m, 4096, 4096, False, qdtype, F32)
            yield case(m, 4096, 4096, True, qdtype, F16)


def group_quant_cases():
    """The experts' int8 product: every leg of its route (ragged weight stream at the three tile heights, 128-row tiles, the
    256 x 256 kernel row-staged, direct and split, the generic kernel), then the switches that force a leg."""
    def case(groups, m, k, n, odtype=BF16, tag="", **env):
        def run():
            x, w = _tensor((m, k), torch.int8), _tensor((groups, n, k), torch.int8)
            s_in, s_w = _tensor((m,), F32), _tensor((groups, n), BF16)
            counts = torch.full((groups,), m // groups, dtype=torch.int32)
            counts[0] += m - int(counts.sum())
            counts = counts.to(DEV)
            out = torch.empty(m, n, dtype=odtype, device=DEV)
            lib = L.load()
            with switch_env(**env):
                ws = torch.empty(lib.mojo_hip_group_quant_gemm_workspace_bytes(m, k, n, groups), dtype=torch.uint8, device=DEV)
                L.check(lib.mojo_hip_group_quant_gemm(L.ptr(x), L.ptr(w), L.ptr(s_in), L.ptr(s_w), L.ptr(out), L.ptr(counts), 0,
                                                      m, k, n, groups, 1, L.dtype_code(odtype), L.ptr(ws), ws.numel(),
                                                      L.stream_of(x)), "group_quant_gemm")
            return out

        def workspace():
            with switch_env(**env):
                return L.load().mojo_hip_group_quant_gemm_workspace_bytes(m, k, n, groups)
        return f"{str(odtype)[6:]}:{groups}g:{m}x{k}x{n}{':' + tag if tag else ''}", run, workspace

    for groups, m, k, n in ((4, 64, 256, 64), (4, 100, 256, 64), (4, 256, 256, 64),        # ragged: 16-, 32-, 64-row tiles
                            (4, 400, 128, 128),                                             # 128-row tiles (mean 100 rows, K % 256 != 0)
                            (8, 2048, 256, 4096),                                           # 128 tiles of 256 x 256: unsplit
                            (8, 1032, 1024, 4096),                                          # 80 tiles over 8 K-tiles: split
                            (4, 400, 96, 128)):                                             # K % 128 != 0: generic
        yield case(groups, m, k, n)
    for odtype in (F16, F32):
        yield case(8, 2048, 256, 4096, odtype)
        yield case(8, 1032, 1024, 4096, odtype)
        yield case(4, 400, 128, 128, odtype)
    for tag, tile128, splitk in (("256", "0", "1"), ("tile128", "1", None), ("tile128x256", "256", None), ("splitk", "0", "3"),
                                 ("default", None, None)):                                  # (test_hip_quant_moe.py: TILE_LEGS)
        yield case(8, 2048, 256, 4096, BF16, tag, MOJO_HIP_GEMM_TILE128=tile128, MOJO_HIP_GEMM_SPLITK=splitk)
    yield case(4, 64, 256, 64, BF16, "skinny29", MOJO_HIP_GEMM_SKINNY="29")                 # the ragged bit off
    yield case(8, 1032, 1024, 4096, BF16, "splitk40", MOJO_HIP_GEMM_SPLITK="40")            # a forced split past the K-tiles
    yield case(8, 2048, 256, 4096, BF16, "nostage", MOJO_HIP_GEMM_STAGE_ROWS="0")


CASES = {"gemm": gemm_cases, "gemm_residual_rmsnorm": resnorm_cases, "qkv_rope_store": qkv_cases,
         "gemm_swiglu": swiglu_cases, "quant_gemm": quant_cases, "group_quant_gemm": group_quant_cases}


def routes(op):
    out = {name: [launches_of(run), workspace()] for name, run, workspace in CASES[op]()}
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("op", sorted(CASES))
def test_routes_match_the_table(op):
    with open(TABLE) as f:
        want = json.load(f)[op]
    got = routes(op)
    assert sorted(got) == sorted(want), "the case grid differs from the table's"
    moved = [f"{name}: {got[name]} (table: {want[name]})" for name in sorted(want) if got[name] != want[name]]
    assert not moved, f"{len(moved)} of {len(want)} cases moved:\n" + "\n".join(moved[:40])


if __name__ == "__main__":
    with open(TABLE) as f:
        table = json.load(f) if sys.argv[1:] else {}
    table.update({op: routes(op) for op in sorted(sys.argv[1:] or CASES)})
    with open(TABLE, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{TABLE}: {sum(len(v) for v in table.values())} cases")
