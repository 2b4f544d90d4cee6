"""`MojoPrefillNSA` / `MojoPagedPrefillNSA` (`NSA_PREFILL_OPS`): the core goldens against the fp64 model of
tests/nsa_prefill_golden.py without a GPU, and `HIPPrefillNSA` / `HIPPagedPrefillNSA` (csrc/nsa_prefill.hip) against it on one."""
import sys
import types

import pytest
import torch

import mojo_opset_amd as mo
from mojo_opset_amd.backends.hip import lib as L
from mojo_opset_amd.backends.hip.operators.nsa import HIPPagedPrefillNSA, HIPPrefillNSA
from mojo_opset_amd.core.acc import check_tol_diff
from nsa_prefill_golden import CFG, HEADS, SEQS, TorchPagedPrefillNSA, TorchPrefillNSA, build, model, paged, run, with_gate

gpu = pytest.mark.gpu
UNIT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
FULL = tuple(s for s in SEQS if s[0] == s[1])              # what the contiguous op can take: kv_len = q_len


def check(got, out64, c, dtype):
    """The hard bound is the reference's ``atol = rtol = 1e-2``; the printed figure is decode's bound ``u |out64| + 2^-12 max|V|``,
    which the one rounding of W to 16 bits alone exceeded (5.20 bf16, 1.09 fp16) and the residual product on steps with a large
    weight brings back inside.  Measured on an MI355X over the graded cases: at most 0.92 of that bound (bf16) and 0.61 (fp16);
    the equal-keys cases 0.25 - 0.76."""
    got = got.cpu().double()
    assert not torch.isnan(got).any()
    bound = UNIT[dtype] * out64.abs() + 2.0 ** -12 * torch.nan_to_num(c["value"].double()).abs().max()
    print(f"max |err| / (u |out64| + 2^-12 max|V|) = {((got - out64).abs() / bound).max():.3f}")
    check_tol_diff(got, out64, atol=1e-2, rtol=1e-2)


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("page", [None, 16, 128])
def test_core_golden_is_within_the_reference_tolerance_of_the_fp64_model(page, causal):
    """Unplanted, ``nsel >= nb`` for every row: nothing discrete."""
    cfg = tuple(dict(CFG, num_selected_blocks=3).items())
    c = build(64, torch.bfloat16, seqs=FULL[:3] if page is None else SEQS[:4], cfg=cfg, plant=False, causal=causal)
    op = (TorchPrefillNSA if page is None else TorchPagedPrefillNSA)(HEADS, 64, is_causal=causal, **dict(cfg))
    check_tol_diff(run(op, c, page).double(), c["out64"], atol=1e-2, rtol=1e-2)


def test_sets_constructor_and_plugin():
    assert mo.NSA_PREFILL_OPS == mo.core.NSA_PREFILL_OPS == mo.core.operators.NSA_PREFILL_OPS == ("MojoPrefillNSA", "MojoPagedPrefillNSA")
    assert not set(mo.NSA_PREFILL_OPS) & set(mo.__all__)
    op = TorchPagedPrefillNSA(8, 128)
    assert (op.compress_ratio, op.num_selected_blocks, op.block_size, op.window_size, op.is_causal) == (4, 16, 64, 512, True)
    assert tuple(op.gate_proj.shape) == (8, 128, 3) and "window_size=512" in repr(op)
    from mojo_opset_amd import plugin

    ref = types.ModuleType("stand_in_nsa_prefill_reference")
    cores = {n: type(n, (mo.core.MojoOperator,), {"forward": lambda self, *a, **k: None}) for n in mo.NSA_PREFILL_OPS}
    vars(ref).update(cores)
    sys.modules[ref.__name__] = ref
    try:
        made = plugin.rebase_hip_backend(ref, platforms=["rocm", "cpu"])
    finally:
        del sys.modules[ref.__name__]
    for name, hip in (("MojoPrefillNSA", HIPPrefillNSA), ("MojoPagedPrefillNSA", HIPPagedPrefillNSA)):
        assert issubclass(made[name], cores[name]) and made[name].forward is hip.forward


@pytest.mark.parametrize("name", ["head_dim 96", "bs % cr", "page 8", "nsel 65", "int8 caches"])
def test_refusals_come_before_any_device_work(name):
    """CPU tensors: a refusal that came behind the first device step would be the loader's `MojoHipError` instead."""
    dim = 96 if name == "head_dim 96" else 64
    cfg = dict(CFG, **{"bs % cr": dict(compress_ratio=5), "nsel 65": dict(num_selected_blocks=65)}.get(name, {}))
    c = build(dim, torch.bfloat16, seqs=((20, 20),), heads=2, plant=False)
    kc, vc, table = paged(c, 8 if name == "page 8" else 16)
    if name == "int8 caches":
        kc, vc = torch.zeros_like(kc, dtype=torch.int8), torch.zeros_like(vc, dtype=torch.int8)
    with pytest.raises(NotImplementedError):
        with_gate(HIPPagedPrefillNSA(2, dim, **cfg), c)(c["query"], kc, vc, c["cu_q"], table)
    if name not in ("page 8", "int8 caches"):
        with pytest.raises(NotImplementedError):
            with_gate(HIPPrefillNSA(2, dim, **cfg), c)(c["query"], c["key"][0], c["value"][0], c["cu_q"])


@gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("page", [None, 16, 128])
@pytest.mark.parametrize("dim", [64, 128])
def test_kernel_against_the_fp64_model(dim, page, dtype, monkeypatch):
    """The graded cases, causal.  Decode's bound, printed by `check`: 0.85 - 0.92 (bf16) and 0.46 - 0.61 (fp16) on an MI355X."""
    c = build(dim, dtype, seqs=FULL if page is None else SEQS)
    monkeypatch.setenv("MOJO_BACKEND", "hip")
    op = (mo.MojoPrefillNSA if page is None else mo.MojoPagedPrefillNSA)(HEADS, dim, **CFG)
    assert type(op) is (HIPPrefillNSA if page is None else HIPPagedPrefillNSA)
    got = run(op, c, page, "cuda")
    assert L.last_launch() == f"nsa_prefill:w4:d{dim}"
    check(got, c["out64"], c, dtype)
    assert torch.equal(run(op, c, page, "cuda"), got), "two calls differ"


@gpu
@pytest.mark.parametrize("page,seq,causal", [(None, (192, 192), True), (16, (40, 192), True), (16, (5, 192), False)])
def test_visible_key_set_and_ties(page, seq, causal):
    """All keys equal and V[t] = 8 e_(t mod D): every softmax is uniform, equal block scores take blocks 0 and 1, and an
    off-by-one at a causal, window, group or block edge moves an element by at least 8 g / 48."""
    c = dict(build(64, torch.bfloat16, seqs=(seq,), heads=2, plant=False, causal=causal))
    c["key"] = c["key"][:, :1].expand_as(c["key"]).contiguous()
    c["value"] = (8.0 * torch.eye(64)[torch.arange(seq[1]) % 64])[None, :, None, :].expand_as(c["value"]).to(torch.bfloat16).contiguous()
    op = (HIPPrefillNSA if page is None else HIPPagedPrefillNSA)(2, 64, is_causal=causal, **CFG)
    check(run(op, c, page, "cuda"), model(c), c, torch.bfloat16)


@gpu
def test_a_table_that_turns_negative_halfway_reads_zero_rows(monkeypatch):
    c = build(64, torch.bfloat16)
    key, value = c["key"].clone(), c["value"].clone()
    key[6, 96:], value[6, 96:] = 0, 0                        # sequence 6 (33 over 200), pages of 16: -1 from page 6 on
    want = model(c, key, value)
    monkeypatch.setenv("MOJO_HIP_VALIDATE", "1")             # the first page id is valid: no error
    mo.switches.reload()
    try:
        check(run(HIPPagedPrefillNSA(HEADS, 64, **CFG), c, 16, "cuda", hole=(6, 6)), want, c, torch.bfloat16)
        with pytest.raises(ValueError):
            run(HIPPagedPrefillNSA(HEADS, 64, **CFG), c, 16, "cuda", hole=(6, 0))
    finally:
        monkeypatch.delenv("MOJO_HIP_VALIDATE")
        mo.switches.reload()


@gpu
@pytest.mark.parametrize("page", [None, 64])
def test_reference_shape_against_the_core_golden(page):
    """Unplanted data, every block taken (nothing discrete): the reference's own test, its shape and its tolerance.

    Measured on an MI355X, both layouts: max |kernel - fp64| = 0.0147, max |golden - fp64| = 0.0319, max |kernel - golden| = 0.0312
    (without the residual product one element of 262144 missed: 0.0117 where 0.0114 is allowed)."""
    cfg = dict(CFG, num_selected_blocks=4, block_size=64, window_size=64)
    c = build(64, torch.bfloat16, seqs=((256, 256), (256, 256)), heads=8, cfg=tuple(cfg.items()), plant=False)
    hip, core = (HIPPrefillNSA, TorchPrefillNSA) if page is None else (HIPPagedPrefillNSA, TorchPagedPrefillNSA)
    got, want = run(hip(8, 64, **cfg), c, page, "cuda").cpu(), run(core(8, 64, **cfg), c, page)
    print(f"max |kernel - fp64| = {(got.double() - c['out64']).abs().max():.4f}, max |golden - fp64| = "
          f"{(want.double() - c['out64']).abs().max():.4f}, max |kernel - golden| = {(got.double() - want.double()).abs().max():.4f}")
    check_tol_diff(got, want, atol=1e-2, rtol=1e-2)
