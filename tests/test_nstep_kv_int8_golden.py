"""The n-step paged decode over the int8 cache (`MojoPagedDecodeNstepSWAWithKVDequant`) without a GPU: the golden against
the prefill golden (bit for bit) and against the single-step golden (one rounding step), dispatch and registration,
`NSTEP_KV_INT8_OPS`, the plugin, constructor and forward errors, and the C workspace query."""
import types

import pytest
import torch

import mojo_opset_amd as mo
import nstep_kv_int8_golden as NG
import oracle.kv_int8 as G
import oracle.kv_int8_swa as SWA
from mojo_opset_amd.core.platform import get_platform

NAME = "MojoPagedDecodeNstepSWAWithKVDequant"
WINDOWS = [(None, None), (4, None), (None, 5), (4, 5)]        # (global, local): none, either, both


def inputs(kv_lens, steps, hq=8, hkv=2, d=64, page=16, dtype=torch.bfloat16, seed=0):
    g = torch.Generator().manual_seed(seed)
    need = [(n + page - 1) // page for n in kv_lens]
    total = sum(need) + 3
    k8, ks = G.quantize_kv_cache(torch.randn(total, hkv, page, d, generator=g))
    v8, vs = G.quantize_kv_cache(torch.randn(total, hkv, page, d, generator=g))
    table = torch.full((len(kv_lens), max(max(need), 1)), -1, dtype=torch.int32)
    free = torch.randperm(total, generator=g, dtype=torch.int32)
    at = 0
    for b, n in enumerate(need):
        table[b, :n] = free[at: at + n]
        at += n
    q = torch.randn(len(kv_lens), steps, hq, d, generator=g).to(dtype)
    return q, k8, ks, v8, vs, torch.tensor(kv_lens, dtype=torch.int32), table


def golden(cls, dtype, **kw):
    op = cls(**kw)
    op.query_dtype = dtype                 # (the constructor admits bf16 only; the forward's math is dtype-generic)
    return op


def cu(lens):
    return torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist(), dtype=torch.int32)


@pytest.fixture(scope="module")
def cases():
    """(constructor kwargs, inputs, n-step golden's output) over dtypes, layouts, windows and S = 1..4, computed once."""
    out = []
    for dtype in (torch.bfloat16, torch.float16):
        for layout in ("AABB", "ABAB"):
            for glob, local in WINDOWS:
                for steps in (1, 2, 3, 4):
                    kw = dict(gqa_layout=layout, global_window_size=glob, local_window_size=local)
                    args = inputs([37, 16 + steps, steps, 0, 130], steps, dtype=dtype, seed=steps)
                    q, k8, ks, v8, vs, lens, table = args
                    got = golden(NG.TorchPagedDecodeNstepSWAWithKVDequant, dtype, **kw).forward(q, None, k8, ks, v8, vs, lens, table)
                    out.append((kw, dtype, args, got))
    return out


def test_golden_is_the_prefill_golden_on_s_rows_bit_for_bit(cases):
    for kw, dtype, (q, k8, ks, v8, vs, lens, table), got in cases:
        steps = q.shape[1]
        live = [b for b, n in enumerate(lens.tolist()) if n > 0]
        rows = torch.cat([q[b] for b in live])
        q_lens = [steps if n > 0 else 0 for n in lens.tolist()]
        pre = golden(SWA.TorchPagedPrefillSWAWithKVDequant, dtype, **kw)
        want = pre.forward(rows, None, k8, ks, v8, vs, cu(q_lens), table, cu_total_seq_lens=cu(lens.tolist()))
        full = torch.zeros_like(q)
        for i, b in enumerate(live):
            full[b] = want[i * steps: (i + 1) * steps]
        assert torch.equal(got, full), (kw, dtype, steps)
        assert not bool(got[3].any()) and bool(torch.isfinite(got.float()).all())


def test_step_j_is_the_single_step_golden_within_one_rounding_step(cases):
    """Not bit for bit: the fp32 ``bmm`` sums in another order for 1 and for ``S`` rows.  atol = rtol = 2^-7, one bf16
    rounding step."""
    for kw, dtype, (q, k8, ks, v8, vs, lens, table), got in cases:
        steps = q.shape[1]
        single = golden(SWA.TorchPagedDecodeSWAWithKVDequant, dtype, **kw)
        for j in range(steps):
            lens_j = torch.where(lens > 0, lens - (steps - 1 - j), lens)
            want = single.forward(q[:, j].contiguous(), None, k8, ks, v8, vs, lens_j, table)
            torch.testing.assert_close(got[:, j].float(), want.float(), atol=2.0 ** -7, rtol=2.0 ** -7)


def test_dispatch_registers_torch_and_hip():
    core = getattr(mo, NAME)
    assert core.get_backend_impl("torch", strict=True) is NG.TorchPagedDecodeNstepSWAWithKVDequant
    from mojo_opset_amd.backends import hip

    assert issubclass(hip.HIPPagedDecodeNstepSWAWithKVDequant, core)
    if get_platform() == "rocm":
        assert core.get_backend_impl("hip", strict=True) is hip.HIPPagedDecodeNstepSWAWithKVDequant


def test_the_name_is_in_a_set_of_its_own():
    assert tuple(mo.NSTEP_KV_INT8_OPS) == (NAME,)
    assert getattr(mo, NAME).__name__ == NAME and NAME not in mo.__all__
    for other in (mo.EXTENDED_OPS, mo.KV_INT8_OPS, mo.KV_INT8_SWA_OPS, mo.QUANT_MOE_OPS, mo.SAMPLING_OPS,
                  mo.BEYOND_SURVEY_OPS, mo.NSTEP_OPS):
        assert NAME not in other
    assert len(mo.BEYOND_SURVEY_OPS) == 16 and tuple(mo.NSTEP_OPS) == ("MojoPagedDecodeNstepSWA",)


def test_constructor_and_repr_are_those_of_the_windowed_int8_pair():
    cls = NG.TorchPagedDecodeNstepSWAWithKVDequant
    op = cls(gqa_layout="ABAB", global_window_size=4, local_window_size=255)
    twin = SWA.TorchPagedDecodeSWAWithKVDequant(gqa_layout="ABAB", global_window_size=4, local_window_size=255)
    names = ("is_causal", "gqa_layout", "gqa_interleave", "global_window_size", "local_window_size", "query_dtype",
             "context_dtype", "compute_dtype")
    assert [getattr(op, n) for n in names] == [True, "ABAB", True, 4, 255, torch.bfloat16, torch.int8, torch.bfloat16]
    assert op.extra_repr() == twin.extra_repr()
    assert (cls(compute_dtype=torch.int8).qmax, cls(compute_dtype=torch.int8).qmin) == (127, -128)
    with pytest.raises(ValueError):
        cls(gqa_layout="BBAA")
    with pytest.raises(NotImplementedError):
        cls(query_dtype=torch.int8)


def _me(**kw):
    base = dict(is_causal=True, gqa_layout="AABB", gqa_interleave=False, global_window_size=None, local_window_size=None,
                query_dtype=torch.bfloat16, context_dtype=torch.int8, compute_dtype=torch.bfloat16)
    return types.SimpleNamespace(**{**base, **kw})


def test_host_refusals_need_no_gpu():
    from mojo_opset_amd.backends.hip import HIPPagedDecodeNstepSWAWithKVDequant as Hip
    from mojo_opset_amd.backends.hip.lib import MojoHipError

    q, k8, ks, v8, vs, lens, table = inputs([5], 2)
    rest = (k8, ks, v8, vs, lens, table)
    with pytest.raises(AssertionError, match="4D query"):
        Hip.forward(_me(), q[:, 0], None, *rest)
    with pytest.raises(AssertionError, match="4D query"):
        NG.TorchPagedDecodeNstepSWAWithKVDequant().forward(q[:, 0], None, *rest)
    with pytest.raises(NotImplementedError, match="causal"):
        Hip.forward(_me(is_causal=False), q, None, *rest)
    with pytest.raises(NotImplementedError, match="compute_dtype"):
        Hip.forward(_me(compute_dtype=torch.int8), q, None, *rest)
    with pytest.raises(NotImplementedError, match="quantised queries"):
        Hip.forward(_me(), q, torch.ones(1, 2, 8, 1), *rest)
    with pytest.raises(NotImplementedError, match="quantised queries"):
        Hip.forward(_me(), q.to(torch.int8), None, *rest)
    for glob, local in [(0, None), (-1, 4), (None, -3)]:
        with pytest.raises(ValueError):
            Hip.forward(_me(global_window_size=glob, local_window_size=local), q, None, *rest)
    with pytest.raises(MojoHipError, match="CPU tensor"):
        Hip.forward(_me(), q, None, *rest)


def test_rebase_walks_the_set_and_skips_a_name_the_reference_lacks():
    """`plugin.rebase_hip_backend` walks ``NSTEP_KV_INT8_OPS`` too: a reference with a class of the name gets the hip
    backend grafted on, today's reference (no such class) is skipped."""
    import sys

    from mojo_opset_amd import plugin
    from mojo_opset_amd.backends import hip
    from mojo_opset_amd.core import MojoOperator

    for with_class in (True, False):
        ref = types.ModuleType(f"stand_in_nstep_kv_int8_reference_{int(with_class)}")
        exp = types.ModuleType(ref.__name__ + ".experimental")
        core = type(NAME, (MojoOperator,), {"forward": lambda self, *a, **k: None, "__module__": exp.__name__})
        if with_class:
            setattr(exp, NAME, core)
        sys.modules[ref.__name__], sys.modules[exp.__name__] = ref, exp
        try:
            made = plugin.rebase_hip_backend(ref, platforms=["rocm", "cpu"])
        finally:
            del sys.modules[ref.__name__], sys.modules[exp.__name__]
        assert (NAME in made) == with_class
        if with_class:
            cls = made[NAME]
            assert cls.__name__ == "HIPPagedDecodeNstepSWAWithKVDequant" and issubclass(cls, core)
            assert cls.forward is hip.HIPPagedDecodeNstepSWAWithKVDequant.forward
            assert "__init__" not in vars(cls)


def test_workspace_query_answers_without_a_gpu(monkeypatch):
    from mojo_opset_amd.backends.hip import lib as L

    lib = L.load()
    query = lib.mojo_hip_paged_decode_nstep_kv8_workspace_bytes
    assert query(5, 8, 2, 128, 16, 20, 0, -1, 0, 4) >= 0
    assert query(5, 8, 1, 128, 48, 20, 0, 255, 4, 3) >= 0            # pages of 48, two blocks of steps
    assert query(5, 8, 2, 96, 16, 20, 0, -1, 0, 4) >= 0
    # not geometries of the int8 kernel: a group of 32, a page of 8, a head_dim without an instance; no steps
    assert query(5, 32, 1, 128, 16, 20, 0, -1, 0, 4) == -1
    assert query(5, 8, 2, 128, 8, 40, 0, -1, 0, 4) == -1
    assert query(5, 8, 2, 112, 16, 20, 0, -1, 0, 4) == -1
    assert query(5, 8, 2, 128, 16, 20, 0, -1, 0, 0) == -1
    geom = (64, 32, 8, 128, 16, 256, 0)
    for windows in [(-1, 0), (4095, 0), (255, 4)]:
        assert query(*geom, *windows, 1) == lib.mojo_hip_paged_decode_swa_kv8_workspace_bytes(*geom, *windows)
    assert query(*geom, -1, 0, 4) >= query(*geom, -1, 0, 1) > 0     # 16 columns per (sequence, kv head) instead of 4
    monkeypatch.setenv("MOJO_HIP_DECODE_MFMA", "0")                   # the composed route's switch
    assert query(5, 8, 2, 128, 16, 20, 0, -1, 0, 4) == -1
