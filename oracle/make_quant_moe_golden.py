"""Write tests/golden/quant_moe.pt: reference outputs of the W8A8 MoE ops (authoring machine only).

Usage: python oracle/make_quant_moe_golden.py [reference root]   (default: MOJO_REFERENCE_ROOT, else /root/reference; nothing else reads it)

The outputs come from the reference's own ``torch`` backends of `MojoMoEDynamicQuant`
(`mojo_opset/core/operators/quantize.py:178-247`), `MojoQuantExperts` (`core/operators/moe.py:452-667`) and `MojoQuantMoE`
(`:132-274`), built on CPU and loaded with the recorded state.  Each case records the constructor keywords, the state, the
inputs and the output; tests/test_quant_moe_golden.py pins oracle/quant_moe.py to them bit for bit (both forms of
the integer product) and tests/test_hip_quant_moe.py runs the hip backend on them.

The int8 expert weights dominate the file, so every int8 case uses ONE weight set (E 4, H 128, I 192; torch.save stores a
shared tensor once); the int4 / group-scale case has a smaller one of its own.
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.quant_moe import pack_int4  # noqa: E402

E, H, I = 4, 128, 192


def quantize_rows(w, q_max, group=-1):
    """Symmetric per-output-row quantisation of ``w [..., N, K]`` (per K group of ``group`` columns when > 0):
    scale = amax / q_max, values rounded and clamped to [-q_max - 1, q_max] -> (int8 values, fp32 scales [..., N] or [..., N, groups])."""
    parts = w.float().split(group, dim=-1) if group > 0 else [w.float()]
    q, s = [], []
    for p in parts:
        scale = (p.abs().amax(dim=-1, keepdim=True) / q_max).clamp(min=1e-12)
        q.append(torch.round(p / scale).clamp(-q_max - 1, q_max).to(torch.int8))
        s.append(scale)
    scales = torch.cat(s, dim=-1)
    return torch.cat(q, dim=-1), (scales if group > 0 else scales.squeeze(-1))


def ep_counts(g, experts, tokens, top_k, dtype):
    """Counts drawn the way the reference's test draws them: ids over 2 * experts, the upper half dropped (the EP case)."""
    ids = torch.randint(0, 2 * experts, (tokens, top_k), generator=g)
    return torch.bincount(ids.flatten(), minlength=2 * experts)[:experts].to(dtype)


def main(reference_root):
    sys.path.insert(0, reference_root)
    import mojo_opset as ref

    g = torch.Generator().manual_seed(2031)
    up8, up_s = quantize_rows(torch.randn(E, 2 * I, H, generator=g) * 0.1, 127)
    down8, down_s = quantize_rows(torch.randn(E, H, I, generator=g) * 0.1, 127)
    up_s, down_s = up_s.bfloat16(), down_s.bfloat16()
    cases = []

    def smooth(experts, dim):
        return 1.0 / (torch.rand(experts, dim, generator=g) + 0.5)

    def record(op, kwargs, state, args):
        cls = getattr(ref, op)._registry.get("torch")
        mod = cls(**kwargs)
        mod.load_state_dict({k: v.clone() for k, v in state.items()})
        with torch.no_grad():
            out = mod(*[a.clone() for a in args])
        cases.append({"op": op, "ctor": {"kwargs": kwargs}, "state": state, "args": tuple(args), "kwargs": {}, "out": out})

    # ---- MojoMoEDynamicQuant: three input dtypes, both count dtypes, an empty expert ----
    for dtype, cdtype, shape, counts in [(torch.float32, torch.int64, (12, H), [4, 3, 5, 0]),
                                         (torch.bfloat16, torch.int32, (21, H), [2, 5, 0, 14]),
                                         (torch.float16, torch.int32, (9, I), [0, 9, 0, 0])]:
        x = torch.randn(*shape, generator=g).to(dtype)
        record("MojoMoEDynamicQuant", {"expert_num": E, "input_size": shape[-1]}, {"inv_smooth_scale": smooth(E, shape[-1])},
               [x, torch.tensor(counts, dtype=cdtype)])

    # ---- MojoQuantExperts, int8 / per-channel ----
    def experts_state(u8, us, d8, ds, hidden, inter):
        return {"up_proj_weight": u8, "down_proj_weight": d8, "up_proj_weight_scale": us, "down_proj_weight_scale": ds,
                "up_proj_quantize.inv_smooth_scale": smooth(u8.shape[0], hidden), "down_proj_quantize.inv_smooth_scale": smooth(u8.shape[0], inter)}

    for dtype, counts in [(torch.bfloat16, ep_counts(g, E, 33, 2, torch.int32)),          # the reference test's EP-style counts
                          (torch.float16, torch.tensor([5, 0, 9, 3], dtype=torch.int64)),   # an expert with zero rows
                          (torch.bfloat16, torch.tensor([0, 0, 17, 0], dtype=torch.int32))]:  # one expert holds every row
        x = torch.randn(int(counts.sum()), H, generator=g).to(dtype)
        record("MojoQuantExperts", {"num_experts": E, "hidden_size": H, "intermediate_size": I},
               experts_state(up8, up_s, down8, down_s, H, I), [x, counts])

    # ---- MojoQuantExperts, int4 weights with group scales (golden only: the hip class refuses them) ----
    e4, h4, i4, gu, gd = 3, 64, 96, 32, 48
    u4, u4s = quantize_rows(torch.randn(e4, 2 * i4, h4, generator=g) * 0.1, 7, gu)
    d4, d4s = quantize_rows(torch.randn(e4, h4, i4, generator=g) * 0.1, 7, gd)
    counts = torch.tensor([4, 0, 7], dtype=torch.int32)
    record("MojoQuantExperts", {"num_experts": e4, "hidden_size": h4, "intermediate_size": i4, "up_quant_group_size": gu,
                                "up_weight_dtype": "int4", "down_quant_group_size": gd, "down_weight_dtype": "int4"},
           experts_state(pack_int4(u4), u4s.bfloat16(), pack_int4(d4), d4s.bfloat16(), h4, i4),
           [torch.randn(11, h4, generator=g).to(torch.bfloat16), counts])

    # ---- MojoQuantMoE: top-k 2 and 4 ----
    for dtype, top_k, tokens in [(torch.bfloat16, 2, 33), (torch.float16, 4, 19)]:
        state = {"experts." + k: v for k, v in experts_state(up8, up_s, down8, down_s, H, I).items()}
        state["gating.gate_weight"] = torch.randn(H, E, generator=g) * 0.2
        record("MojoQuantMoE", {"num_experts": E, "top_k": top_k, "hidden_size": H, "intermediate_size": I}, state,
               [torch.randn(tokens, H, generator=g).to(dtype)])

    path = os.path.join(ROOT, "tests", "golden", "quant_moe.pt")
    torch.save({"cases": cases}, path)
    print(path, os.path.getsize(path), "bytes,", len(cases), "cases")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("MOJO_REFERENCE_ROOT", "/root/reference"))
