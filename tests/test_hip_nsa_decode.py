"""`MojoDecodeNSA` / `MojoPagedDecodeNSA` (`NSA_ATTN_OPS`): the core goldens against the fp64 model of tests/nsa_golden.py without
a GPU, and `HIPDecodeNSA` / `HIPPagedDecodeNSA` (csrc/nsa_decode.hip) against the same model on one."""
import sys
import types

import pytest
import torch

import mojo_opset_amd as mo
from mojo_opset_amd.backends.hip import lib as L
from mojo_opset_amd.backends.hip.operators.nsa import HIPDecodeNSA, HIPPagedDecodeNSA
from mojo_opset_amd.core.acc import check_tol_diff
from nsa_golden import CFG, HEADS, TorchDecodeNSA, TorchPagedDecodeNSA, build, model, paged, with_gate

gpu = pytest.mark.gpu
UNIT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


def run(op, c, page, device="cpu", hole=None, **kw):
    """Case ``c`` through ``op``: contiguous K/V for ``page`` None, else caches of that page size."""
    op = with_gate(op, c, device)
    if page is None:
        return op(c["query"].to(device), c["key"].to(device), c["value"].to(device), c["lens"].to(device), **kw)
    kc, vc, table = paged(c, page, hole)
    return op(c["query"].to(device), kc.to(device), vc.to(device), c["lens"].to(device), table.to(device), **kw)


def within_bound(got, out64, c, dtype):
    """|got - out64| <= u |out64| + 2^-12 max|V|: the one output rounding, plus about 8 x what fp32 scores (D 2^-24 |q||k|), the
    hardware exponential and an fp32 sum over about 1000 keys can move an output.  Measured on an MI355X over every case of
    this file: at most 0.74 of the bound (bf16) and 0.37 (fp16), the same in both forms and on every layout — above half, and
    the cause is the output rounding alone: ``u |out64|`` IS the largest error of one rounding to nearest, and no element's
    error exceeds that first term (the second printed figure, the share of the second term an element needs, is never
    above 0.000)."""
    got = got.cpu().double()
    assert not torch.isnan(got).any()
    err, rounding = (got - out64).abs(), UNIT[dtype] * out64.abs()
    second = 2.0 ** -12 * torch.nan_to_num(c["value"].double()).abs().max()
    print(f"max |err| / bound = {(err / (rounding + second)).max():.3f}, max (|err| - u |out64|) / second term = "
          f"{((err - rounding) / second).max():.3f}")
    assert bool((err <= rounding + second).all())


@pytest.mark.parametrize("page", [None, 16, 128])
def test_core_golden_is_within_the_reference_tolerance_of_the_fp64_model(page):
    c = build(64, torch.bfloat16)
    op = (TorchDecodeNSA if page is None else TorchPagedDecodeNSA)(HEADS, 64, **CFG)
    check_tol_diff(run(op, c, page).double(), c["out64"], atol=1e-2, rtol=1e-2)


def test_sets_constructor_and_plugin():
    assert mo.NSA_ATTN_OPS == mo.core.NSA_ATTN_OPS == mo.core.operators.NSA_ATTN_OPS == ("MojoDecodeNSA", "MojoPagedDecodeNSA")
    assert not set(mo.NSA_ATTN_OPS) & set(mo.__all__)
    op = TorchPagedDecodeNSA(8, 128)
    assert (op.compress_ratio, op.num_selected_blocks, op.block_size, op.window_size, op.is_causal) == (4, 16, 64, 512, True)
    assert tuple(op.gate_proj.shape) == (8, 128, 3) and "window_size=512" in repr(op)
    from mojo_opset_amd import plugin

    ref = types.ModuleType("stand_in_nsa_reference")
    cores = {n: type(n, (mo.core.MojoOperator,), {"forward": lambda self, *a, **k: None}) for n in mo.NSA_ATTN_OPS}
    vars(ref).update(cores)
    sys.modules[ref.__name__] = ref
    try:
        made = plugin.rebase_hip_backend(ref, platforms=["rocm", "cpu"])
    finally:
        del sys.modules[ref.__name__]
    for name, hip in (("MojoDecodeNSA", HIPDecodeNSA), ("MojoPagedDecodeNSA", HIPPagedDecodeNSA)):
        assert issubclass(made[name], cores[name]) and made[name].forward is hip.forward


@pytest.mark.parametrize("name", ["head_dim 96", "bs % cr", "page 8", "nsel 65", "int8 caches"])
def test_refusals_come_before_any_device_work(name):
    """CPU tensors: a refusal that came behind the first device step would be the loader's `MojoHipError` instead."""
    dim = 96 if name == "head_dim 96" else 64
    cfg = dict(CFG, **{"bs % cr": dict(compress_ratio=5), "nsel 65": dict(num_selected_blocks=65)}.get(name, {}))
    c = build(dim, torch.bfloat16, lens=(20,), heads=2, plant=False)
    kc, vc, table = paged(c, 8 if name == "page 8" else 16)
    if name == "int8 caches":
        kc, vc = torch.zeros_like(kc, dtype=torch.int8), torch.zeros_like(vc, dtype=torch.int8)
    with pytest.raises(NotImplementedError):
        with_gate(HIPPagedDecodeNSA(2, dim, **cfg), c)(c["query"], kc, vc, c["lens"], table)
    if name not in ("page 8", "int8 caches"):
        with pytest.raises(NotImplementedError):
            with_gate(HIPDecodeNSA(2, dim, **cfg), c)(c["query"], c["key"], c["value"], c["lens"])


@gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("num_splits", [1, 3])
@pytest.mark.parametrize("page", [None, 16, 128])
@pytest.mark.parametrize("dim", [64, 128])
def test_kernel_against_the_fp64_model(dim, page, num_splits, dtype, monkeypatch):
    c = build(dim, dtype)
    monkeypatch.setenv("MOJO_BACKEND", "hip")
    op = (mo.MojoDecodeNSA if page is None else mo.MojoPagedDecodeNSA)(HEADS, dim, **CFG)
    assert type(op) is (HIPDecodeNSA if page is None else HIPPagedDecodeNSA)
    got = run(op, c, page, "cuda", num_splits=num_splits)
    assert L.last_launch() == (f"nsa_decode:fused:d{dim}" if num_splits == 1 else f"nsa_decode:split3:d{dim}")
    within_bound(got, c["out64"], c, dtype)
    assert torch.equal(run(op, c, page, "cuda", num_splits=num_splits), got), "two calls of one form differ"
    planned = run(op, c, page, "cuda")
    form = L.last_launch()
    first = got if form.startswith("nsa_decode:fused") else run(op, c, page, "cuda", num_splits=int(form.split(":")[1][5:]))
    assert torch.equal(planned, first), f"the planned call ({form}) differs from the forced call of its form"


@gpu
@pytest.mark.parametrize("page", [None, 64])
def test_reference_shape_against_the_core_golden(page):
    """Unplanted data, every block taken (nothing discrete): the reference's own test, its shape and its tolerance."""
    cfg = dict(CFG, num_selected_blocks=4, block_size=64, window_size=64)
    c = build(64, torch.bfloat16, lens=(256, 256), heads=8, cfg=tuple(cfg.items()), plant=False)
    hip, core = (HIPDecodeNSA, TorchDecodeNSA) if page is None else (HIPPagedDecodeNSA, TorchPagedDecodeNSA)
    check_tol_diff(run(hip(8, 64, **cfg), c, page, "cuda").cpu(), run(core(8, 64, **cfg), c, page), atol=1e-2, rtol=1e-2)


@gpu
@pytest.mark.parametrize("num_splits", [1, 3])
def test_equal_block_scores_take_the_lower_index(num_splits):
    """All keys equal, V constant within a block and distinct between blocks, six blocks, two taken: blocks 0 and 1."""
    c = dict(build(64, torch.bfloat16, lens=(6 * 32,), heads=2, plant=False))
    c["key"] = c["key"][:, :1].expand_as(c["key"]).contiguous()
    c["value"] = (torch.arange(6 * 32) // 32 - 2.5)[None, :, None, None].expand_as(c["value"]).to(torch.bfloat16).contiguous()
    got = run(HIPDecodeNSA(2, 64, **CFG), c, None, "cuda", num_splits=num_splits)
    within_bound(got, model(c), c, torch.bfloat16)


@gpu
def test_a_table_that_turns_negative_halfway_reads_zero_rows(monkeypatch):
    c = build(64, torch.bfloat16)
    key, value = c["key"].clone(), c["value"].clone()
    key[4, 512:], value[4, 512:] = 0, 0                      # sequence 4 (1030 keys), pages of 16: -1 from page 32 on
    want = model(c, key, value)
    monkeypatch.setenv("MOJO_HIP_VALIDATE", "1")             # the first page id is valid: no error
    mo.switches.reload()
    try:
        for num_splits in (1, 3):
            within_bound(run(HIPPagedDecodeNSA(HEADS, 64, **CFG), c, 16, "cuda", hole=(4, 32), num_splits=num_splits), want, c,
                         torch.bfloat16)
        with pytest.raises(ValueError):
            run(HIPPagedDecodeNSA(HEADS, 64, **CFG), c, 16, "cuda", hole=(4, 0))
    finally:
        monkeypatch.delenv("MOJO_HIP_VALIDATE")
        mo.switches.reload()
