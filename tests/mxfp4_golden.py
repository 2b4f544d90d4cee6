"""fp64 models of the MXFP4 ops (`MXFP4_OPS`) and the case builders of tests/test_hip_mxfp4.py.  Written from the format's rules
(core/operators/mxfp4.py's docstring), not from the core code: the exponent through ``log2``, the rounding as a nearest-value search
over the grid with the tie going to the even code."""
import functools

import torch

GRID = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=torch.float64)
TIES = (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)                              # each goes to the neighbour with the even code
TIE_CODES = (0, 2, 2, 4, 4, 6, 6)


def quant_model64(x):
    """``x [M, K]`` -> ``(data, scale)`` uint8, block by block in fp64."""
    m, k = x.shape
    xb = x.double().reshape(m, k // 32, 32)
    bad = ~torch.isfinite(xb).all(-1)
    amax = torch.where(bad, torch.ones((), dtype=torch.float64), xb.abs().amax(-1))
    e = torch.where(amax > 0, torch.floor(torch.log2(amax.clamp_min(2.0 ** -200))) - 2, torch.full_like(amax, -127.0)).clamp(-127, 127)
    y = (xb.abs() * torch.pow(torch.tensor(2.0, dtype=torch.float64), -e).unsqueeze(-1)).clamp_max(6.0)
    dist = (y.unsqueeze(-1) - GRID).abs()
    nearest = dist == dist.amin(-1, keepdim=True)                          # one code, or two neighbours on a tie
    even = torch.arange(8) % 2 == 0
    code = torch.where((nearest & even).any(-1), (nearest & even).int().argmax(-1), nearest.int().argmax(-1))
    nibble = (code + 8 * torch.signbit(xb).int()).to(torch.uint8)
    nibble = torch.where(bad.unsqueeze(-1), torch.zeros_like(nibble), nibble).reshape(m, k)
    scale = torch.where(bad, torch.full_like(e, 255.0), e + 127).to(torch.uint8)
    return nibble[:, 0::2] | (nibble[:, 1::2] << 4), scale


def dequant_model64(data, scale):
    """fp64 ``[M, K]`` of ``(data [M, K/2], scale [M, K/32])``."""
    nibble = torch.stack((data & 0xF, data >> 4), -1).reshape(data.shape[0], -1).long()
    value = torch.where(nibble >= 8, -GRID[nibble % 8], GRID[nibble % 8])
    factor = torch.pow(torch.tensor(2.0, dtype=torch.float64), scale.double() - 127)
    return (value.reshape(data.shape[0], -1, 32) * factor.unsqueeze(-1)).reshape(data.shape[0], -1)


def gemm_model64(a, sa, w, sw):
    """``(product, sum_k |a_k b_k|)`` in fp64."""
    a64, w64 = dequant_model64(a, sa), dequant_model64(w, sw)
    return a64 @ w64.T, a64.abs() @ w64.abs().T


@functools.lru_cache(maxsize=None)
def operand(rows, k, lo, hi, seed):
    """Random nibbles and scale bytes uniform in ``[lo, hi]``, a fresh scale for every block: ``(data, scale)``."""
    gen = torch.Generator().manual_seed(seed * 7919 + rows * 31 + k)
    data = torch.randint(0, 256, (rows, k // 2), generator=gen, dtype=torch.uint8)
    scale = torch.randint(lo, hi + 1, (rows, k // 32), generator=gen).to(torch.uint8)
    return data, scale


def quant_input(m, k, dtype, seed=0):
    """Rows for the quantiser: per-block magnitudes over a wide range, and in the leading blocks every tie in both signs, a
    saturating block (second-largest value in (6, 8) of the scaled range), zeros of both signs, subnormals, the largest finite
    value, an Inf block and a NaN block."""
    gen = torch.Generator().manual_seed(seed + 13 * m + k)
    spread = 20 if dtype == torch.bfloat16 else 6
    x = torch.randn(m, k // 32, 32, generator=gen) * torch.pow(2.0, torch.randint(-spread, spread + 1, (m, k // 32, 1), generator=gen).float())
    special = special_blocks(dtype)
    flat = x.reshape(-1, 32)
    n = min(len(special), flat.shape[0])
    flat[:n] = special[:n]
    return flat.reshape(m, k).to(dtype)


def special_blocks(dtype):
    tiny = torch.finfo(dtype).tiny
    ties = torch.tensor(TIES + tuple(-t for t in TIES))
    blocks = torch.zeros(6, 32)
    blocks[0, :14], blocks[0, 14] = ties, 4.0                              # amax 4: e = 0, the ties as they stand
    blocks[1, :14], blocks[1, 14] = ties * 2.0 ** -9, 7.5 * 2.0 ** -9      # amax 7.5 * 2^-9: e = -9, the block's largest saturates
    blocks[2, 0], blocks[2, 1], blocks[2, 2], blocks[2, 3] = 7.75, -7.0, 6.5, 5.0   # the second-largest in (6, 8): saturates too
    blocks[3, 1], blocks[3, 5] = -0.0, -0.0                                # a zero block keeps its signs
    blocks[4, 0], blocks[4, 1], blocks[4, 2] = tiny / 4, -tiny / 2, tiny / 64       # subnormals only
    blocks[5, 0], blocks[5, 1] = torch.finfo(dtype).max, -1.0
    inf, nan = torch.ones(2, 32), torch.ones(2, 32)
    inf[0, 3], inf[1, 0], nan[0, 31], nan[1, 7] = float("inf"), -float("inf"), float("nan"), float("nan")
    return torch.cat([blocks, inf, nan])
