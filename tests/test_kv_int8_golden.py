"""The int8 paged KV cache ops without a GPU: the goldens against the recorded reference outputs, dispatch, constructor
errors and `extra_repr`, `KV_INT8_OPS`, the plugin's registration, the host-side refusals of the hip classes and the
workspace entry points.

The recorded outputs (oracle/make_kv_int8_golden.py) are three files — store, decode, prefill — each under the 1 MiB
bound of a committed file."""
import types

import pytest
import torch

import mojo_opset_amd as mo
import oracle.kv_int8
from conftest import bit_equal, build_op, clone_tree, load_golden
from mojo_opset_amd.core import MojoOperator
from mojo_opset_amd.core.platform import get_platform

KV8_OPS = ("MojoStorePagedKVCacheC8", "MojoPagedDecodeGQAWithKVDequant", "MojoPagedPrefillGQAWithKVDequant")
ATTN_OPS = KV8_OPS[1:]
STORE, DECODE, PREFILL = (load_golden("paged_kv_int8_" + n) for n in ("store", "decode", "prefill"))
CASES = STORE + DECODE + PREFILL


@pytest.mark.parametrize("case", [pytest.param(c, id=f"{c['op'][4:]}-{i}") for i, c in enumerate(CASES)])
def test_golden_reproduces_the_reference_bit_for_bit(case):
    op = build_op(getattr(oracle.kv_int8, "Torch" + case["op"][4:]), case)
    out = op.forward(*clone_tree(case["args"]), **clone_tree(case["kwargs"]))
    assert bit_equal(out, case["out"])


def test_fixtures_cover_what_they_must():
    attn = [(c["ctor"]["kwargs"], c["args"]) for c in DECODE + PREFILL]
    assert {k["gqa_layout"] for k, _ in attn} == {"AABB", "ABAB"}
    assert {a[0].shape[1] // a[2].shape[1] for _, a in attn} >= {1, 2, 4, 8}            # groups
    assert {a[0].shape[2] for _, a in attn} >= {64, 96, 128}                            # head_dim
    assert {a[2].shape[2] for _, a in attn} >= {16, 32, 128}                            # pages
    for cases in (DECODE, PREFILL):
        assert any(c["ctor"]["kwargs"]["compute_dtype"] == torch.int8 for c in cases)
        assert any(c["ctor"]["kwargs"]["compute_dtype"] == torch.bfloat16 for c in cases)
    assert any(0 in c["args"][6].tolist() for c in DECODE)                               # a zero-length row
    assert any(int(c["kwargs"]["cu_total_seq_lens"][-1]) > int(c["args"][6][-1]) for c in PREFILL)   # a cached prefix
    assert {c["args"][4].dtype for c in STORE} >= {torch.bfloat16, torch.float32}       # scale dtypes
    assert any("chunk_metadata" in c["kwargs"] for c in STORE) and any(len(c["args"]) == 9 for c in STORE)
    legacy = [c["args"] for c in STORE if len(c["args"]) == 9]
    assert any(a[7] is None for a in legacy) and any(a[7] is not None for a in legacy)   # decode and prefill mode
    assert any(-1 in a[8].tolist() for a in legacy)
    assert any(a[7] is not None and 0 in (a[7][1:] - a[7][:-1]).tolist() for a in legacy)
    for c in STORE:
        for s in c["args"][4:6]:
            assert bool((s != 0).all()) and bool((s < 0).any()) and bool((s > 0).any())


@pytest.mark.parametrize("name", KV8_OPS)
def test_dispatch_registers_torch_and_hip(name):
    core = getattr(mo, name)
    assert core.get_backend_impl("torch", strict=True).__name__ == "Torch" + name[4:]
    from mojo_opset_amd.backends import hip

    hip_cls = getattr(hip, "HIP" + name[4:])
    assert issubclass(hip_cls, core)
    if get_platform() == "rocm":
        assert core.get_backend_impl("hip", strict=True) is hip_cls


def test_kv_int8_ops_are_attributes_but_not_in_all_or_extended_ops():
    assert tuple(mo.KV_INT8_OPS) == KV8_OPS
    assert tuple(mo.EXTENDED_OPS) == ("MojoPagedDecodeSWA", "MojoPagedPrefillSWA")
    for name in KV8_OPS:
        assert name not in mo.__all__ and getattr(mo, name).__name__ == name
    assert len(mo.__all__) == len(set(mo.__all__))


@pytest.mark.parametrize("name", ATTN_OPS)
def test_constructor_and_repr_follow_the_reference(name):
    cls = getattr(oracle.kv_int8, "Torch" + name[4:])
    op = cls(gqa_layout="ABAB")
    assert (op.is_causal, op.gqa_layout, op.query_dtype, op.context_dtype, op.compute_dtype) == \
        (True, "ABAB", torch.bfloat16, torch.int8, torch.bfloat16)
    assert not hasattr(op, "qmax")
    assert op.extra_repr() == ("is_causal=True, gqa_layout='ABAB', query_dtype=torch.bfloat16, context_dtype=torch.int8, "
                               "compute_dtype=torch.bfloat16")
    q8 = cls(compute_dtype=torch.int8)
    assert (q8.qmax, q8.qmin) == (127, -128)
    with pytest.raises(ValueError):
        cls(gqa_layout="BBAA")
    with pytest.raises(NotImplementedError):
        cls(query_dtype=torch.int8)
    with pytest.raises(AssertionError):
        cls(context_dtype=torch.bfloat16)
    with pytest.raises(AssertionError):
        cls(compute_dtype=torch.float16)


def _decode_inputs():
    q = torch.zeros(1, 2, 64, dtype=torch.bfloat16)
    k = torch.zeros(2, 1, 16, 64, dtype=torch.int8)
    s = torch.ones(1, 64, dtype=torch.bfloat16)
    return q, k, s, k.clone(), s.clone(), torch.tensor([5], dtype=torch.int32), torch.tensor([[0, -1]], dtype=torch.int32)


def _me(**over):
    kw = dict(is_causal=True, gqa_layout="AABB", query_dtype=torch.bfloat16, context_dtype=torch.int8,
              compute_dtype=torch.bfloat16)
    kw.update(over)
    return types.SimpleNamespace(**kw)


@pytest.mark.parametrize("what", ["compute_int8", "mask", "non_causal", "query_scale", "head_dim", "not_dense"])
def test_unbuilt_paths_raise_before_any_device_work(what):
    """Everything that is not built raises `NotImplementedError` from `HIP*.forward` on CPU tensors: it needs neither a
    GPU nor a sync."""
    from mojo_opset_amd.backends.hip import HIPPagedDecodeGQAWithKVDequant, HIPPagedPrefillGQAWithKVDequant

    q, k, ks, v, vs, lens, table = _decode_inputs()
    me, qs, kwargs = _me(), None, {}
    if what == "compute_int8":
        me = _me(compute_dtype=torch.int8, qmax=127, qmin=-128)
    elif what == "mask":
        kwargs = {"mask": torch.ones(8, 8, dtype=torch.bool)}
    elif what == "non_causal":
        me = _me(is_causal=False)
    elif what == "query_scale":
        qs = torch.ones(1, 2, 1, dtype=torch.bfloat16)
    elif what == "head_dim":
        q, k, ks = torch.zeros(1, 2, 32, dtype=torch.bfloat16), torch.zeros(2, 1, 16, 32, dtype=torch.int8), ks[:, :32]
        v, vs = k.clone(), ks.clone()
    elif what == "not_dense":
        k = torch.zeros(2, 1, 16, 128, dtype=torch.int8)[..., ::2]
        v = k.clone()
    with pytest.raises(NotImplementedError):
        HIPPagedDecodeGQAWithKVDequant.forward(me, q, qs, k, ks, v, vs, lens, table, **kwargs)
    with pytest.raises(NotImplementedError):
        HIPPagedPrefillGQAWithKVDequant.forward(me, q, qs, k, ks, v, vs, torch.tensor([0, 1], dtype=torch.int32), table, **kwargs)


def test_store_refuses_what_is_not_built_on_the_host():
    from mojo_opset_amd.backends.hip import HIPStorePagedKVCacheC8

    me = types.SimpleNamespace(check_call_contract=mo.MojoStorePagedKVCacheC8.check_call_contract)
    kc = torch.zeros(2, 1, 16, 64, dtype=torch.int8)
    s = torch.ones(1, 64, dtype=torch.bfloat16)
    plan = torch.tensor([[0, 0, 0, 1]], dtype=torch.int32)
    x = torch.zeros(1, 1, 64, dtype=torch.float32)
    with pytest.raises(NotImplementedError):                 # fp32 states
        HIPStorePagedKVCacheC8.forward(me, x, x.clone(), kc, kc.clone(), s, s.clone(), chunk_metadata=plan)
    x = x.to(torch.bfloat16)
    with pytest.raises(NotImplementedError):                 # a cache that is not dense in head_dim
        wide = torch.zeros(2, 1, 16, 128, dtype=torch.int8)[..., ::2]
        HIPStorePagedKVCacheC8.forward(me, x, x.clone(), wide, wide.clone(), s, s.clone(), chunk_metadata=plan)
    with pytest.raises(AssertionError):                      # plan and legacy arguments mixed
        HIPStorePagedKVCacheC8.forward(me, x, x.clone(), kc, kc.clone(), s, s.clone(), torch.zeros(1, 2, dtype=torch.int32),
                                       chunk_metadata=plan)


def test_workspace_entry_points_answer_without_a_gpu():
    from mojo_opset_amd.backends.hip import lib as L

    lib = L.load()
    # headline decode: B 64, 32 q / 8 kv heads, D 128, page 16, ctx 4096 -> 4 chunks per row, fp32 partials [D + 2]
    dec = lib.mojo_hip_paged_decode_gqa_kv8_workspace_bytes(64, 32, 8, 128, 16, 256, 4096)
    assert dec == 64 * 8 * 4 * 4 * 130 * 4 + 256
    assert lib.mojo_hip_paged_decode_gqa_kv8_workspace_bytes(0, 32, 8, 128, 16, 256, 4096) == 0
    # prefill: the scratch holds batch * ceil(min(hint, page * width) / page) 16-bit pages of K and of V (+ table, + split)
    pages = 2 * 128
    pool = pages * 8 * 16 * 128 * 2
    pf = lib.mojo_hip_paged_prefill_gqa_kv8_workspace_bytes(4096, 2, 32, 8, 128, 16, 1024, 2048, 2048)
    assert 2 * pool <= pf <= 2 * pool + (64 << 20)
    wide = lib.mojo_hip_paged_prefill_gqa_kv8_workspace_bytes(4096, 2, 32, 8, 128, 16, 1024, 2048, 0)
    assert wide >= 2 * 8 * pool                               # no hint: the table's capacity (1024 pages per row)
    assert lib.mojo_hip_paged_prefill_gqa_kv8_workspace_bytes(0, 2, 32, 8, 128, 16, 1024, 0, 0) == 0


def test_rebase_registers_all_three_classes_into_a_stand_in_reference():
    """`plugin.rebase_hip_backend` walks ``KV_INT8_OPS`` too, and finds the classes in ``<reference>.experimental``."""
    import sys

    from mojo_opset_amd import plugin
    from mojo_opset_amd.backends import hip

    ref = types.ModuleType("stand_in_reference_kv8")
    exp = types.ModuleType("stand_in_reference_kv8.experimental")
    ref.experimental = exp
    sys.modules[ref.__name__], sys.modules[exp.__name__] = ref, exp
    try:
        def ctor(self, *args, **kwargs):
            MojoOperator.__init__(self)

        for name in KV8_OPS:
            core = type(name, (MojoOperator,), {"__init__": ctor, "forward": lambda self, *a, **k: None,
                                                "__module__": exp.__name__})
            setattr(exp, name, core)
        made = plugin.rebase_hip_backend(ref, platforms=["rocm", "cpu"])
        for name in KV8_OPS:
            cls = made[name]
            assert cls.__name__ == "HIP" + name[4:] and issubclass(cls, getattr(exp, name))
            assert cls.forward is getattr(hip, "HIP" + name[4:]).forward
            assert "__init__" not in vars(cls)
    finally:
        del sys.modules[ref.__name__], sys.modules[exp.__name__]
