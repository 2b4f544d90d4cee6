"""`MojoPagedPrefillSageGQA` (`SAGE_ATTN_OPS`): the core golden against the fp64 model of tests/sage_golden.py without a GPU, and
`HIPPagedPrefillSageGQA` (csrc/sage_prefill.hip) against the same model on one."""
import functools
import sys
import types

import pytest
import torch

import mojo_opset_amd as mo
from mojo_opset_amd.backends.hip.operators.sage import HIPPagedPrefillSageGQA
from sage_golden import TorchPagedPrefillSageGQA, build, call, model

gpu = pytest.mark.gpu
Q_LENS, CACHED = [1, 70, 33, 0], [130, 0, 31, 5]


@functools.lru_cache(maxsize=None)
def case(dim, page, hq, hkv, q_lens=tuple(Q_LENS), cached=tuple(CACHED)):
    c = build(dim, page, hq, hkv, list(q_lens), list(cached))
    return c, {layout: model(c, layout) for layout in ("AABB", "ABAB")}


@pytest.mark.parametrize("layout", ["AABB", "ABAB"])
@pytest.mark.parametrize("geom", [(128, 16, 4, 2, (37, 5), (0, 43)), (64, 32, 8, 2, (1, 70, 33), (130, 0, 31))], ids=str)
def test_core_golden_is_the_fp64_model_bit_for_bit(geom, layout):
    c, want = case(*geom)
    got = call(TorchPagedPrefillSageGQA(gqa_layout=layout), c)
    assert got.dtype == torch.bfloat16 and torch.equal(got, want[layout][0].to(torch.bfloat16))


def test_sets_constructor_and_plugin():
    assert mo.SAGE_ATTN_OPS == mo.core.SAGE_ATTN_OPS == mo.core.operators.SAGE_ATTN_OPS == ("MojoPagedPrefillSageGQA",)
    with pytest.raises(AssertionError):
        TorchPagedPrefillSageGQA(compute_dtype=torch.bfloat16)
    from mojo_opset_amd import plugin

    ref = types.ModuleType("stand_in_sage_reference")
    core = type("MojoPagedPrefillSageGQA", (mo.core.MojoOperator,), {"forward": lambda self, *a, **k: None})
    ref.MojoPagedPrefillSageGQA = core
    sys.modules[ref.__name__] = ref
    try:
        made = plugin.rebase_hip_backend(ref, platforms=["rocm", "cpu"])
    finally:
        del sys.modules[ref.__name__]
    assert issubclass(made["MojoPagedPrefillSageGQA"], core)
    assert made["MojoPagedPrefillSageGQA"].forward is HIPPagedPrefillSageGQA.forward


def _refusals():
    c = case(128, 16, 4, 2, (37, 5), (0, 43))[0]
    wide = dict(c, block_tables=torch.full((2, 132104 // 16 + 1), -1, dtype=torch.int32))
    bad_dim = build(96, 16, 4, 2, [3], [0])
    bad_page = build(128, 8, 4, 2, [3], [0])
    return {"mask": (c, {}, dict(mask=torch.ones(1, 1, dtype=torch.bool))), "not causal": (c, dict(is_causal=False), {}),
            "D=96": (bad_dim, {}, {}), "page=8": (bad_page, {}, {}), "bf16 query": (dict(c, query=c["query"].bfloat16()), {}, {}),
            "wide table, no hint": (wide, {}, {})}


@pytest.mark.parametrize("name", ["mask", "not causal", "D=96", "page=8", "bf16 query", "wide table, no hint"])
def test_refusals_come_before_any_device_work(name):
    """CPU tensors: a refusal that came behind the first device step would be the loader's `MojoHipError` instead."""
    c, ctor, kw = _refusals()[name]
    with pytest.raises(NotImplementedError):
        call(HIPPagedPrefillSageGQA(**ctor), c, **kw)


@gpu
@pytest.mark.parametrize("layout", ["AABB", "ABAB"])
@pytest.mark.parametrize("group", [1, 4])
@pytest.mark.parametrize("page", [16, 64])
@pytest.mark.parametrize("dim", [64, 128])
def test_kernel_against_the_fp64_model(dim, page, group, layout, monkeypatch):
    """|got - out64| <= 2^-7 |out64| + 256 value_scale / S: one bf16 step, plus what one probability rounding the other way
    (numerator by at most 128, divisor by 1) moves a row; at most 1 % of the elements may need the second term."""
    hkv = 2
    c, want = case(dim, page, hkv * group, hkv)
    out64, sums = want[layout]
    monkeypatch.setenv("MOJO_BACKEND", "hip")
    op = mo.MojoPagedPrefillSageGQA(gqa_layout=layout)
    assert type(op) is HIPPagedPrefillSageGQA
    got = call(op, c, "cuda", max_q_len=max(Q_LENS), max_total_seq_len=max(a + b for a, b in zip(Q_LENS, CACHED)))
    again = call(op, c, "cuda")
    assert got.dtype == torch.bfloat16 and torch.equal(got, again), "two calls (with and without hints) differ"
    got = got.cpu().double()
    assert not torch.isnan(got).any()
    heads = torch.arange(hkv * group)
    vs = c["value_scale"].double()[heads % hkv if layout == "ABAB" else heads // group]          # [Hq, D]
    err, step = (got - out64).abs(), out64.abs() * 2.0 ** -7
    flip = 256 * vs[None] / sums.clamp_min(1)[:, :, None]
    share = (err > step).double().mean().item()
    print(f"max err {err.max():.3e}, share needing the second term {share:.4%}")
    assert bool((err <= step + flip).all()) and share <= 0.01


def _one_hot():
    c = build(128, 16, 4, 2, [5], [60], seed=1)
    c["key_scale"] = torch.nan_to_num(c["key_scale"], nan=0.0) * 0 + 1e-4          # every score within 0.03 ...
    c["query"][:] = 1
    c["query_scale"][:] = 1.0
    blk, hot = int(c["block_tables"][0, 1]), 3                                       # ... but key 16 + 3: 127 * 128 * 1e-2 * scale
    c["key_cache"][blk, :, hot], c["key_scale"][blk, :, hot] = 127, 1e-2
    want = (c["value_cache"][blk, :, hot].float() * c["value_scale"]).repeat_interleave(2, 0).bfloat16()
    return c, want[None].expand(5, -1, -1)


def _equal_scores():
    c = build(128, 16, 4, 2, [2], [4094], seed=2, extra_width=0)
    c["key_cache"][:], c["key_scale"][:] = 1, 1.0
    c["value_cache"][:] = torch.tensor([127, 126], dtype=torch.int8).repeat(8)[None, None, :, None]
    c["value_scale"][:] = 2.0 ** -5
    c["block_tables"] = torch.arange(256, dtype=torch.int32)[None]                   # pages in order: even keys 127, odd 126
    want = torch.full((2, 4, 128), 126.5 * 2.0 ** -5).bfloat16()
    want[0] = ((127 * 253 * 2047 + 127 * 127) * 2.0 ** -5 / (127 * 4095))            # the first row sees 4095 keys
    return c, want


@gpu
@pytest.mark.parametrize("make", [_one_hot, _equal_scores])
def test_exact_cases(make):
    """One-hot: one score exceeds the rest by more than 6, every other p is 0, out = bf16(v8 * value_scale).  Equal scores:
    4096 keys with p = 127 each, sum p v = 127 * 253 * 2048 > 2^24 - an fp32 accumulator misses 126.5 * 2^-5."""
    c, want = make()
    got = call(HIPPagedPrefillSageGQA(), c, "cuda").cpu()
    assert torch.equal(got, want)
