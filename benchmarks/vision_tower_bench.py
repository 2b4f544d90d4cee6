"""The vision-tower ops (`VISION_TOWER_OPS`) benchmark (standalone; not part of bench.py):
python -m benchmarks.vision_tower_bench

Attention legs in bf16, 20 / 20 heads, head_dim 64 (the reference's vision config), HIP events:

  uniform_16x1024    16 sequences of 1024 tokens (16 images)
  windows_256x64     256 windows of 64 tokens (window attention: one key tile per sequence)
  ragged_16          16 sequences of 256 .. 1024 tokens

Per leg, in one process: ``hip`` the `HIPPackedSdpa`; ``sdpa`` `HIPSdpa` on ``[B, 20, S, 64]`` (uniform lengths, the same FLOPs;
for the ragged leg the uniform_16x1024 tensor, scaled by FLOPs); ``swa_causal`` `HIPSWA` causal on the same tokens (half the
FLOPs); ``torch`` the torch composition (`F.scaled_dot_product_attention` per distinct length).  FLOP/s are reported for all.

RoPE legs: the vision apply on ``[16384, 20, 64]`` q and k and MRoPE (in place and out of place) on 8192 tokens of 28 / 4 heads x
128 with sections [16, 24, 24], each against `HIPApplyRoPE` on the same bytes and against the torch composition of its golden.

Every figure is the median of 5 timed regions after warm-up (min and max beside it).  Judged as benchmarks/dit_block_bench.py
judges: an op may take its sibling's time for its own FLOPs (attention) or bytes (RoPE), plus the sibling's own min-to-max spread
in this run, plus 5 % of the sibling's median (``allowed_us``, ``hip_within_margin``).  One JSON object."""
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from benchmarks.extras import _hbm, _mfma, _time, _want, hip  # noqa: E402

BF16 = torch.bfloat16
HEADS, HEAD_DIM = 20, 64


def _judge(res, work, sibling, sibling_work):
    """``work``: FLOPs or bytes of the op; the sibling's time is scaled to it."""
    sib = res[sibling]
    scale = work / sibling_work
    spread = sib["us_max"] - sib["us_min"]
    res["sibling"], res["sibling_spread_us"] = sibling, spread
    res["allowed_us"] = (sib["us"] + spread + 0.05 * sib["us"]) * scale
    res["hip_minus_sibling_us"] = res["hip"]["us"] - sib["us"] * scale
    res["hip_within_margin"] = res["hip"]["us"] <= res["allowed_us"]
    res["torch_over_hip"] = res["torch"]["us"] / res["hip"]["us"]
    return res


def _cu(lens, device):
    return torch.tensor([0] + [sum(lens[:i + 1]) for i in range(len(lens))], dtype=torch.int32, device=device)


def _torch_attention(q, k, v, lens):
    """The torch composition: one `scaled_dot_product_attention` per run of equal lengths."""
    out, start, i = torch.empty_like(q), 0, 0
    while i < len(lens):
        j = i
        while j < len(lens) and lens[j] == lens[i]:
            j += 1
        n, rows = j - i, (j - i) * lens[i]
        view = lambda t: t[start:start + rows].view(n, lens[i], HEADS, HEAD_DIM).transpose(1, 2)  # noqa: E731
        out[start:start + rows] = F.scaled_dot_product_attention(view(q), view(k), view(v)).transpose(1, 2).reshape(rows, HEADS, HEAD_DIM)
        start, i = start + rows, j
    return out


def attention_cases(device, out):
    packed, sdpa, swa = hip("MojoPackedSdpa")(), hip("MojoSdpa")(), hip("MojoSWA")()
    ragged = [256 + (i * 768) // 15 for i in range(16)]
    uniform = None
    for name, lens in (("uniform_16x1024", [1024] * 16), ("windows_256x64", [64] * 256), ("ragged_16", ragged)):
        if not _want(name):
            continue
        tokens = sum(lens)
        q, k, v = (torch.randn(tokens, HEADS, HEAD_DIM, device=device, dtype=BF16) for _ in range(3))
        cu = _cu(lens, device)
        flops = sum(4.0 * HEADS * HEAD_DIM * n * n for n in lens)
        longest = max(lens)
        res = {"hip": _mfma(_time(lambda: packed(q, k, v, cu, cu, max_q_len=longest, max_total_seq_len=longest)), flops),
               "swa_causal": _mfma(_time(lambda: swa(q, k, v, cu, cu, max_q_len=longest, max_total_seq_len=longest)), flops / 2),
               "torch": _mfma(_time(lambda: _torch_attention(q, k, v, lens)), flops)}
        if len(set(lens)) == 1:
            as4 = lambda t: t.view(len(lens), lens[0], HEADS, HEAD_DIM).transpose(1, 2)  # noqa: E731
            res["sdpa"] = _mfma(_time(lambda: sdpa(as4(q), as4(k), as4(v))), flops)
            sib_flops = flops
            if name == "uniform_16x1024":
                uniform = (res["sdpa"], flops)
        else:                                                # no uniform form of these tokens: the 16 x 1024 launch, scaled by FLOPs
            if uniform is None:
                u = [torch.randn(16, 1024, HEADS, HEAD_DIM, device=device, dtype=BF16).transpose(1, 2) for _ in range(3)]
                uniform = (_mfma(_time(lambda: sdpa(*u)), 16 * 4.0 * HEADS * HEAD_DIM * 1024 * 1024), 16 * 4.0 * HEADS * HEAD_DIM * 1024 * 1024)
            res["sdpa"], sib_flops = uniform
        res["flops"], res["sibling_flops"], res["tokens"] = flops, sib_flops, tokens
        out[name] = _judge(res, flops, "sdpa", sib_flops)
        del q, k, v
    torch.cuda.empty_cache()


def _golden_vision_rope(q, k, cos, sin):
    def turn(x):
        wide, half = x.float(), x.shape[-1] // 2
        rot = torch.cat((-wide[..., half:], wide[..., :half]), dim=-1)
        return (wide * cos.unsqueeze(1) + rot * sin.unsqueeze(1)).to(x.dtype)
    return turn(q), turn(k)


def _golden_mrope(q, k, cos, sin, sec, hd):
    tokens, half = q.shape[0], sum(sec)
    c = torch.cat([m[i] for i, m in enumerate(cos.split(sec, dim=-1))], dim=-1).unsqueeze(1)
    s = torch.cat([m[i] for i, m in enumerate(sin.split(sec, dim=-1))], dim=-1).unsqueeze(1)

    def turn(x):
        h = x.view(tokens, -1, hd)
        h1, h2 = h[..., :half], h[..., half:2 * half]
        return torch.cat([h1 * c - h2 * s, h2 * c + h1 * s, h[..., 2 * half:]], dim=-1).view(tokens, -1).to(x.dtype)
    return turn(q), turn(k)


def rope_cases(device, out):
    apply_rope = hip("MojoApplyRoPE")()
    if _want("vision_rope_16384x20x64"):
        t = 16384
        q, k = (torch.randn(t, HEADS, HEAD_DIM, device=device, dtype=BF16) for _ in range(2))
        cos, sin = torch.randn(t, HEAD_DIM, device=device), torch.randn(t, HEAD_DIM, device=device)
        vision = hip("MojoApplyVisionRoPE2D")()
        nbytes = 2 * (q.numel() + k.numel()) * 2
        res = {"hip": _hbm(_time(lambda: vision(q, k, cos, sin)), nbytes),
               "apply_rope": _hbm(_time(lambda: apply_rope(q, k, cos, sin, head_first=False)), nbytes),
               "torch": _hbm(_time(lambda: _golden_vision_rope(q, k, cos, sin)), nbytes)}
        res["bytes"] = res["sibling_bytes"] = nbytes
        out["vision_rope_16384x20x64"] = _judge(res, nbytes, "apply_rope", nbytes)
    t, hq, hk, hd, sec = 8192, 28, 4, 128, [16, 24, 24]
    q, k = torch.randn(t, hq * hd, device=device, dtype=BF16), torch.randn(t, hk * hd, device=device, dtype=BF16)
    angle = torch.rand(3, t, hd // 2, device=device) * 6.0      # unit phases: the in-place leg rotates the same q again and again
    cos3, sin3 = angle.cos(), angle.sin()
    cos, sin = torch.randn(t, hd, device=device), torch.randn(t, hd, device=device)
    nbytes = 2 * (q.numel() + k.numel()) * 2
    sibling = lambda: apply_rope(q.view(t, hq, hd), k.view(t, hk, hd), cos, sin, head_first=False)  # noqa: E731
    for name, op in (("mrope_8192x28x4x128", hip("MojoMRoPE")()), ("mrope_inplace_8192x28x4x128", hip("MojoMRoPEInplace")(inplace=True))):
        if not _want(name):
            continue
        res = {"hip": _hbm(_time(lambda: op(q, k, cos3, sin3, sec, False, hd)), nbytes),
               "apply_rope": _hbm(_time(sibling), nbytes),
               "torch": _hbm(_time(lambda: _golden_mrope(q, k, cos3, sin3, sec, hd)), nbytes)}
        res["bytes"] = res["sibling_bytes"] = nbytes
        out[name] = _judge(res, nbytes, "apply_rope", nbytes)
    torch.cuda.empty_cache()


def bench(device):
    out = {}
    attention_cases(device, out)
    rope_cases(device, out)
    return out


if __name__ == "__main__":
    print(json.dumps({"vision_tower": bench(torch.device("cuda", 0))}))
