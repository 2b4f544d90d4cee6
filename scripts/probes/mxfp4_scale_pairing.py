"""Which scale byte the scaled fp4 instruction pairs with which block, seen through `HIPMXFP4Gemm` in ONE launch per form:
python scripts/probes/mxfp4_scale_pairing.py [--out profiles/mxfp4_scale_pairing.json]

K = 512 is one super-tile: 16 blocks, lane group g owning blocks 4g .. 4g+3, one instruction per op_sel 0..3.  Activation row m
is one-hot: a single 1.0 (code 2) at element ``e(m)`` of block m, all its scale bytes 127 but block m's, which is 120 + m.  Every
weight row n holds 1.0 everywhere with the scale byte 130 + b on block b.  If data block b meets scale byte b on both sides,
``log2 out[m][n] = (m - 7) + (m + 3)`` for every n; any other pairing of lanes, registers or op_sel bytes gives another power of
two (or a sum of several).  The record lists, per form, the exponent found per block and whether all 16 are the expected ones."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from mojo_opset_amd.backends.hip import lib as L  # noqa: E402
from mojo_opset_amd.backends.hip.operators.mxfp4 import HIPMXFP4Gemm  # noqa: E402


def probe(rows, n=16, k=512):
    a, sa = torch.zeros(rows, k // 2, dtype=torch.uint8), torch.full((rows, k // 32), 127, dtype=torch.uint8)
    for m in range(16):
        element = 32 * m + (5 * m + 3) % 32                       # somewhere else inside the block for every row
        a[m, element // 2] = 0x2 << (4 * (element % 2))
        sa[m, m] = 120 + m
    op = HIPMXFP4Gemm(k, n, torch.float32)
    op.weight = torch.full((n, k // 2), 0x22, dtype=torch.uint8, device="cuda")
    op.weight_scale = (130 + torch.arange(k // 32)).to(torch.uint8).repeat(n, 1).cuda()
    out = op(a.cuda(), sa.cuda()).cpu()
    found = torch.log2(out[:16]).tolist()
    expected = [float(2 * m - 4) for m in range(16)]
    return {"kernel_form": L.last_launch(), "log2_out_per_block": [row[0] for row in found], "expected": expected,
            "as_expected": all(row == [e] * n for row, e in zip(found, expected)), "rows_past_16_zero": not out[16:].any().item()}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ns = ap.parse_args()
    line = json.dumps({"mxfp4_scale_pairing": {"skinny": probe(16), "tile": probe(48)}})
    if ns.out:
        with open(ns.out, "w") as f:
            f.write(line + "\n")
    print(line)
