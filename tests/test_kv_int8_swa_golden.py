"""Sliding-window attention over the int8 paged KV cache without a GPU: the goldens against the recorded reference outputs,
what the fixtures cover, dispatch, `KV_INT8_SWA_OPS`, the plugin's registration, constructor and `extra_repr`, the
host-side refusals of the hip classes and the workspace entry points.

The recorded outputs (oracle/make_kv_int8_swa_golden.py) are two files — decode, prefill — each under the 1 MiB bound of
a committed file."""
import types

import pytest
import torch

import mojo_opset_amd as mo
import oracle.kv_int8_swa
from conftest import bit_equal, build_op, clone_tree, load_golden
from mojo_opset_amd.core import MojoOperator
from mojo_opset_amd.core.platform import get_platform

OPS = ("MojoPagedDecodeSWAWithKVDequant", "MojoPagedPrefillSWAWithKVDequant")
DECODE, PREFILL = (load_golden("paged_kv_int8_swa_" + n) for n in ("decode", "prefill"))
CASES = DECODE + PREFILL


@pytest.mark.parametrize("case", [pytest.param(c, id=f"{c['op'][4:]}-{i}") for i, c in enumerate(CASES)])
def test_golden_reproduces_the_reference_bit_for_bit(case):
    op = build_op(getattr(oracle.kv_int8_swa, "Torch" + case["op"][4:]), case)
    out = op.forward(*clone_tree(case["args"]), **clone_tree(case["kwargs"]))
    assert not torch.isnan(case["out"].float()).any()
    assert bit_equal(out, case["out"])


def test_fixtures_cover_what_they_must():
    assert len(DECODE) == 6 and len(PREFILL) == 6
    attn = [(c["ctor"]["kwargs"], c["args"]) for c in CASES]
    assert {k["gqa_layout"] for k, _ in attn} == {"AABB", "ABAB"}
    assert {a[0].shape[1] // a[2].shape[1] for _, a in attn} >= {1, 2, 4, 8}            # groups
    assert {a[0].shape[2] for _, a in attn} >= {64, 96, 128}                            # head_dim
    assert {a[2].shape[2] for _, a in attn} >= {16, 32, 128}                            # pages
    for cases in (DECODE, PREFILL):
        kws = [c["ctor"]["kwargs"] for c in cases]
        assert {k["compute_dtype"] for k in kws} == {torch.int8, torch.bfloat16}
        wins = [(k["global_window_size"], k["local_window_size"]) for k in kws]
        assert any(g is None and l is not None for g, l in wins)                        # local only
        assert any(g is not None and l is None for g, l in wins)                        # global only
        assert any(g is not None and l is not None for g, l in wins)                    # both
    assert any(c["ctor"]["kwargs"]["local_window_size"] == 0 for c in DECODE)           # the query's own key only
    assert any(0 in c["args"][6].tolist() for c in DECODE)                               # a zero-length row
    assert any(0 in (c["args"][6][1:] - c["args"][6][:-1]).tolist() for c in PREFILL)    # an empty sequence
    assert any(int(c["kwargs"]["cu_total_seq_lens"][-1]) > int(c["args"][6][-1]) for c in PREFILL)   # a cached prefix


@pytest.mark.parametrize("name", OPS)
def test_dispatch_registers_torch_and_hip(name):
    core = getattr(mo, name)
    assert core.get_backend_impl("torch", strict=True).__name__ == "Torch" + name[4:]
    from mojo_opset_amd.backends import hip

    hip_cls = getattr(hip, "HIP" + name[4:])
    assert issubclass(hip_cls, core)
    if get_platform() == "rocm":
        assert core.get_backend_impl("hip", strict=True) is hip_cls


def test_the_new_set_is_an_attribute_and_the_other_sets_are_unchanged():
    assert tuple(mo.KV_INT8_SWA_OPS) == OPS
    for name in OPS:
        assert name not in mo.__all__ and getattr(mo, name).__name__ == name
    assert tuple(mo.EXTENDED_OPS) == ("MojoPagedDecodeSWA", "MojoPagedPrefillSWA")
    assert tuple(mo.KV_INT8_OPS) == ("MojoStorePagedKVCacheC8", "MojoPagedDecodeGQAWithKVDequant",
                                     "MojoPagedPrefillGQAWithKVDequant")
    assert tuple(mo.QUANT_MOE_OPS) == ("MojoMoEDynamicQuant", "MojoQuantExperts", "MojoQuantMoE")
    assert len(mo.SAMPLING_OPS) == 6
    assert len(mo.__all__) == len(set(mo.__all__))


def test_rebase_registers_both_classes_into_a_stand_in_reference():
    """`plugin.rebase_hip_backend` walks ``KV_INT8_SWA_OPS`` too, and finds the classes in ``<reference>.experimental``."""
    import sys

    from mojo_opset_amd import plugin
    from mojo_opset_amd.backends import hip

    ref = types.ModuleType("stand_in_reference_kv8_swa")
    exp = types.ModuleType("stand_in_reference_kv8_swa.experimental")
    ref.experimental = exp
    sys.modules[ref.__name__], sys.modules[exp.__name__] = ref, exp
    try:
        def ctor(self, *args, **kwargs):
            MojoOperator.__init__(self)

        for name in OPS:
            core = type(name, (MojoOperator,), {"__init__": ctor, "forward": lambda self, *a, **k: None,
                                                "__module__": exp.__name__})
            setattr(exp, name, core)
        made = plugin.rebase_hip_backend(ref, platforms=["rocm", "cpu"])
        for name in OPS:
            cls = made[name]
            assert cls.__name__ == "HIP" + name[4:] and issubclass(cls, getattr(exp, name))
            assert cls.forward is getattr(hip, "HIP" + name[4:]).forward
            assert "__init__" not in vars(cls)
    finally:
        del sys.modules[ref.__name__], sys.modules[exp.__name__]


@pytest.mark.parametrize("name", OPS)
def test_constructor_and_repr_follow_the_reference(name):
    cls = getattr(oracle.kv_int8_swa, "Torch" + name[4:])
    op = cls(gqa_layout="ABAB", global_window_size=4, local_window_size=255)
    assert (op.is_causal, op.gqa_layout, op.gqa_interleave, op.global_window_size, op.local_window_size, op.query_dtype,
            op.context_dtype, op.compute_dtype) == (True, "ABAB", True, 4, 255, torch.bfloat16, torch.int8, torch.bfloat16)
    assert not hasattr(op, "qmax")
    assert op.extra_repr() == ("is_causal=True, gqa_layout='ABAB', global_window_size=4, local_window_size=255, "
                               "query_dtype=torch.bfloat16, context_dtype=torch.int8, compute_dtype=torch.bfloat16")
    plain = cls()
    assert (plain.gqa_layout, plain.gqa_interleave, plain.global_window_size, plain.local_window_size) == \
        ("AABB", False, None, None)
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


def _inputs(dim=64, page=16):
    q = torch.zeros(1, 2, dim, dtype=torch.bfloat16)
    k = torch.zeros(2, 1, page, dim, dtype=torch.int8)
    s = torch.ones(1, dim, dtype=torch.bfloat16)
    return q, k, s, k.clone(), s.clone(), torch.tensor([5], dtype=torch.int32), torch.tensor([[0, -1]], dtype=torch.int32)


def _me(**over):
    kw = dict(is_causal=True, gqa_layout="AABB", global_window_size=4, local_window_size=7, query_dtype=torch.bfloat16,
              context_dtype=torch.int8, compute_dtype=torch.bfloat16)
    kw.update(over)
    return types.SimpleNamespace(**kw)


def _forwards():
    from mojo_opset_amd.backends.hip import HIPPagedDecodeSWAWithKVDequant, HIPPagedPrefillSWAWithKVDequant

    return HIPPagedDecodeSWAWithKVDequant.forward, HIPPagedPrefillSWAWithKVDequant.forward


@pytest.mark.parametrize("what", ["compute_int8", "non_causal", "query_scale", "int8_query", "head_dim", "not_dense"])
def test_unbuilt_paths_raise_before_any_device_work(what):
    """Everything that is not built raises `NotImplementedError` from `HIP*.forward` on CPU tensors: it needs neither a
    GPU nor a sync."""
    decode, prefill = _forwards()
    q, k, ks, v, vs, lens, table = _inputs()
    me, qs = _me(), None
    if what == "compute_int8":
        me = _me(compute_dtype=torch.int8, qmax=127, qmin=-128)
    elif what == "non_causal":
        me = _me(is_causal=False)
    elif what == "query_scale":
        qs = torch.ones(1, 2, 1, dtype=torch.bfloat16)
    elif what == "int8_query":
        q = q.to(torch.int8)
    elif what == "head_dim":
        q, k, ks, v, vs, lens, table = _inputs(dim=32)
    elif what == "not_dense":
        k = torch.zeros(2, 1, 16, 128, dtype=torch.int8)[..., ::2]
        v = k.clone()
    with pytest.raises(NotImplementedError):
        decode(me, q, qs, k, ks, v, vs, lens, table)
    with pytest.raises(NotImplementedError):
        prefill(me, q, qs, k, ks, v, vs, torch.tensor([0, 1], dtype=torch.int32), table)


def test_windowed_prefill_needs_pages_of_a_multiple_of_16_tokens():
    """Page 8 is inside the unwindowed op's envelope (a multiple of 4) and outside the windowed one's."""
    _, prefill = _forwards()
    q, k, ks, v, vs, _, table = _inputs(page=8)
    with pytest.raises(NotImplementedError, match="multiple of 16"):
        prefill(_me(), q, None, k, ks, v, vs, torch.tensor([0, 1], dtype=torch.int32), table)


@pytest.mark.parametrize("windows", [(None, -1), (-4, 7), (0, None)])
def test_windows_that_leave_a_row_without_a_key_raise_value_error(windows):
    decode, prefill = _forwards()
    q, k, ks, v, vs, lens, table = _inputs()
    me = _me(global_window_size=windows[0], local_window_size=windows[1])
    with pytest.raises(ValueError):
        decode(me, q, None, k, ks, v, vs, lens, table)
    with pytest.raises(ValueError):
        prefill(me, q, None, k, ks, v, vs, torch.tensor([0, 1], dtype=torch.int32), table)


def test_workspace_entry_points_answer_without_a_gpu():
    from mojo_opset_amd.backends.hip import lib as L

    lib = L.load()
    # ---- prefill: a 512-token chunk, local 1023, global 4, pages of 16 tokens, 32 q / 8 kv heads, D 128
    pf = lib.mojo_hip_paged_prefill_swa_kv8_workspace_bytes
    geom = (512, 1, 32, 8, 128, 16)
    narrow = pf(*geom, 2048, 512, 0, 1023, 4)
    wide = pf(*geom, 4096, 512, 0, 1023, 4)
    assert narrow == wide > 0                                  # it no longer grows with the context
    # the pool: ceil(4 / 16) + ceil((512 + 1023 + 1) / 16) + 2 = 99 pages of K and of V per sequence
    # (+ what the 16-bit SWA prefill asks for on those pages, the scratch table and the rebased lengths)
    pool = 99 * 8 * 16 * 128 * 2
    inner = lib.mojo_hip_paged_prefill_swa_workspace_bytes(*geom, 99, 512, 0, 1023, 4)
    assert 2 * pool <= narrow - inner <= 2 * pool + 4096
    for width in (2048, 4096):
        assert narrow < lib.mojo_hip_paged_prefill_gqa_kv8_workspace_bytes(*geom, width, 512, 0)
    # a context shorter than the window: capped by the unwindowed pages per sequence
    assert pf(*geom, 32, 512, 0, 1023, 4) <= lib.mojo_hip_paged_prefill_gqa_kv8_workspace_bytes(*geom, 32, 512, 0) + 512
    # no window: the unwindowed query
    for args in ((*geom, 2048, 512, 0), (4096, 2, 32, 8, 128, 16, 1024, 2048, 2048), (0, 2, 32, 8, 128, 16, 1024, 0, 0)):
        assert pf(*args, -1, 0) == lib.mojo_hip_paged_prefill_gqa_kv8_workspace_bytes(*args)
    # ---- decode: B 64, 32 / 8 heads, D 128, page 16, a table of 2048 pages (ctx 32768)
    dec = lib.mojo_hip_paged_decode_swa_kv8_workspace_bytes
    plain = lib.mojo_hip_paged_decode_gqa_kv8_workspace_bytes
    head = (64, 32, 8, 128, 16)
    for local, glob in ((4095, 0), (1023, 4), (255, 4), (-1, 20)):
        # decode_swa_cap: the global range rounded up to the 16-token tile + local + 16
        cap = (-(-glob // 16) * 16 if glob > 0 else 0) + (local + 16 if local >= 0 else 0)
        assert dec(*head, 2048, 0, local, glob) == plain(*head, -(-cap // 16), cap)
        assert dec(*head, 2048, 0, local, glob) == dec(*head, 4096, 0, local, glob)
    assert dec(*head, 8, 0, 4095, 0) == plain(*head, 8, 0)     # a window wider than the table's capacity
    assert dec(*head, 2048, 0, -1, 0) == plain(*head, 2048, 0)  # no window
    assert dec(*head, 256, 4096, -1, 0) == plain(*head, 256, 4096)
    assert dec(0, 32, 8, 128, 16, 256, 4096, 255, 4) == 0
