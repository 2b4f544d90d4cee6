"""The short-convolution ops (`SHORT_CONV_OPS`: `MojoCausalConv1dUpdateState`, `MojoCausalConv1d`) without a GPU: the goldens
against the recorded reference outputs, the set and its wiring, dispatch and the plugin, the contract errors of the
`HIP<Op>.forward`s (reached before any device call) and the C header.

The recorded outputs (tests/make_short_conv_golden.py) are one file under 256 KiB."""
import os
import re
import sys
import types

import pytest
import torch

import mojo_opset_amd as mo
import short_conv_golden as G
from conftest import GOLDEN, ROOT, load_golden
from mojo_opset_amd.core import MojoOperator
from mojo_opset_amd.core.platform import get_platform

NAMES = ("MojoCausalConv1dUpdateState", "MojoCausalConv1d")
ENTRY_POINT = "mojo_hip_causal_conv1d"
CASES = load_golden("short_conv")
IDS = [pytest.param(c, id=f"{i}-{c['op']}-{c['label']}") for i, c in enumerate(CASES)]
UPDATE = [c for c in CASES if c["op"] == "MojoCausalConv1dUpdateState"]
FUNCTION = [c for c in CASES if c["op"] == "MojoCausalConv1d"]
ROUNDOFF = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32


def same_bits(a, b):
    """Equal dtype, shape and bit patterns (signed zeros told apart)."""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    as_int = torch.int32 if a.element_size() == 4 else torch.int16
    return torch.equal(a.contiguous().view(as_int), b.contiguous().view(as_int))


def golden_of(case):
    args = G.case_args(case)
    if case["op"] == "MojoCausalConv1dUpdateState":
        hidden, state, weight, bias, act = args
        detail = G.update_state_detail(hidden, state, weight, bias, act)
        return detail, weight.shape[1], act
    kw = {k: v for k, v in case["kwargs"].items() if k != "output_final_state"}
    detail = G.conv1d_detail(*args, **kw)
    return detail, args[1].shape[1], kw.get("activation")


def bound_ratio(ref, detail, width, activation):
    """max over the outputs of ``|ref - golden| / ((W + 2) u (sum |w x| + |b|) c + 2 u |golden|)``: ``u`` the storage type's unit
    roundoff, ``c`` = 1.1 with SiLU (its Lipschitz constant) and 1 without.  The bound covers a reference that rounds every partial
    sum, or the convolution itself, to storage."""
    u = ROUNDOFF[ref.dtype]
    c = 1.1 if activation is not None else 1.0
    gold = detail["out"].double()
    allowed = (width + 2) * u * detail["mag"] * c + 2 * u * gold.abs()
    diff = (ref.double() - gold).abs()
    ratio = torch.where(diff == 0, torch.zeros_like(diff), diff / allowed.clamp_min(1e-300))
    return float(ratio.max()) if ratio.numel() else 0.0


@pytest.mark.parametrize("case", IDS)
def test_recorded_outputs_lie_inside_the_bound(case):
    """Every output of every recording: ``|ref - golden| <= (W + 2) u (sum |w x| + |b|) c + 2 u |golden|``.  The largest ratio
    the recordings reach is 0.446 of the bound (the function op, fp32, the packed batch at W 2: the CPU ``conv1d``'s own fp32
    summation order); fp32 update-state recordings reach 0.441.  In 16 bits the update-state op, which rounds the convolution
    to storage before SiLU, reaches 0.251 (bf16, SiLU, 2 x 64 x 128, W 3) and 0.167 in fp16; the function op, which convolves
    in fp32 and rounds once as the golden does, is bit-equal to it in bf16 and fp16 on every recording."""
    detail, width, act = golden_of(case)
    assert detail["out"].dtype == case["out"].dtype and detail["out"].shape == case["out"].shape
    ratio = bound_ratio(case["out"], detail, width, act)
    print(f"{case['op']} {case['label']}: {ratio:.3f} of the bound")
    assert ratio <= 1.0
    # the fp32 accumulator in the fixed order is itself within W + 2 fp32 roundings of the exact sum
    assert bool(((detail["pre"].double() - detail["exact"]).abs() <= (width + 2) * 2.0 ** -24 * detail["mag"]).all())


@pytest.mark.parametrize("case", [pytest.param(c, id=c["label"]) for c in UPDATE])
def test_update_state_results_are_bit_identical(case):
    detail, _, _ = golden_of(case)
    assert same_bits(detail["state"], case["state_after"])
    hidden, state, weight, bias, act = G.case_args(case)
    out = G.TorchCausalConv1dUpdateState().forward(hidden, state, weight, bias, act)       # the class writes in place
    assert same_bits(state, case["state_after"]) and same_bits(out, detail["out"])


@pytest.mark.parametrize("case", [pytest.param(c, id=c["label"]) for c in FUNCTION if c["kwargs"].get("output_final_state")])
def test_final_states_follow_the_recordings(case):
    """Bit-identical to the reference's function wherever its rule and ours agree (no initial state, or a sequence of at least
    ``W - 1`` tokens); with an initial state, bit-identical to what the reference's UPDATE-STATE op leaves on the same
    concatenation - the short sequences included, where the reference's function drops the initial state."""
    detail, width, _ = golden_of(case)
    x = G.case_args(case)[0]
    kw = case["kwargs"]
    out, final = G.TorchCausalConv1d().forward(*G.case_args(case), **kw)
    assert same_bits(final, detail["final_state"]) and same_bits(out, detail["out"])
    cu = kw.get("cu_seqlens")
    spans = [(b, 0, x.shape[1]) for b in range(x.shape[0])] if cu is None else [(0, int(cu[n]), int(cu[n + 1])) for n in range(cu.numel() - 1)]
    rows = case.get("final_state_rows", list(range(len(spans))))
    assert case["final_state"].shape[0] == len(rows)
    for recorded, n in zip(case["final_state"], rows):
        row, bos, eos = spans[n]
        assert same_bits(recorded, G.reference_final_state(x[row, bos:eos], width))         # the reference's rule, restated
        if kw.get("initial_state") is None or eos - bos >= width - 1:
            assert same_bits(final[n], recorded), n
    if kw.get("initial_state") is not None:
        assert same_bits(final, case["state_by_update_op"])
        for n, (row, bos, eos) in enumerate(spans):
            if eos == bos:
                assert same_bits(final[n], kw["initial_state"][n])


def test_the_deviation_is_recorded_and_differs():
    case = next(c for c in FUNCTION if c["label"] == "state-t1-w4-bf16")
    detail, _, _ = golden_of(case)
    assert not same_bits(detail["final_state"], case["final_state"])                         # T = 1 < W - 1 = 3
    assert same_bits(detail["final_state"], case["state_by_update_op"])
    assert same_bits(detail["final_state"][..., :2], case["kwargs"]["initial_state"][..., 1:])   # the initial state shifts in
    assert not case["final_state"][..., :2].any()                                            # the reference pads with zeros
    agree = next(c for c in FUNCTION if c["label"] == "state-t1-w2-bf16")                    # T = 1 = W - 1
    assert same_bits(golden_of(agree)[0]["final_state"], agree["final_state"])


def test_fixture_is_small_and_covers_the_cases():
    assert os.path.getsize(os.path.join(GOLDEN, "short_conv.pt")) < 256 * 1024
    assert {c["op"] for c in CASES} == set(NAMES)
    shape = lambda c: (tuple(G.case_args(c)[0].shape), G.case_args(c)[2 if c in UPDATE else 1].shape[1])  # noqa: E731
    assert ((2, 128, 64), 3) in {shape(c) for c in UPDATE} and ((1, 32, 32), 4) in {shape(c) for c in UPDATE}    # [B, D, T]
    assert ((2, 128, 128), 4) in {shape(c) for c in FUNCTION}
    combos = {(c["args"][2].shape[1], c["args"][1].shape[2], G.case_args(c)[0].shape[2]) for c in UPDATE}       # (W, S, T)
    assert {w for w, _, _ in combos} == {2, 3, 4}
    assert any(s == w - 1 for w, s, _ in combos) and any(s == w for w, s, _ in combos) and any(s == 7 for _, s, _ in combos)
    assert any(t == 1 for _, _, t in combos) and any(1 < t < s for _, s, t in combos) and any(t == s for _, s, t in combos)
    for cases in (UPDATE, FUNCTION):
        assert {G.case_args(c)[0].dtype for c in cases} == {BF16, F16, F32}
    assert {c["args"][3] is None for c in UPDATE} == {True, False}                                                   # bias
    assert {c["args"][4] for c in UPDATE} == {None, "silu", "swish"}
    assert {c["kwargs"].get("activation") for c in FUNCTION} == {None, "silu", "swish"}
    assert any(c["kwargs"].get("residual") is not None for c in FUNCTION)
    assert any(c["kwargs"].get("initial_state") is not None and c["kwargs"].get("output_final_state") for c in FUNCTION)
    packed = [c for c in FUNCTION if c["kwargs"].get("cu_seqlens") is not None]
    assert packed and all(torch.diff(c["kwargs"]["cu_seqlens"]).tolist() == [1, 2, 3, 17, 0, 40] for c in packed)
    assert {c["kwargs"]["cu_seqlens"].dtype for c in packed} == {torch.int32, torch.int64}
    assert {c["kwargs"].get("initial_state") is None for c in packed} == {True, False}
    assert {G.case_args(c)[0].dtype for c in packed} == {BF16, F16, F32} and {c["args"][1].shape[1] for c in packed} == {2, 3, 4}


def test_the_fixed_order_is_what_the_golden_states():
    """64 x 64 fp32 outputs, W 4: a fused multiply-add or the taps summed newest first changes some of them, so a backend that
    is bit-identical to the golden follows the stated order; and the accumulator starts at +0.0, so a lone -0.0 product gives +0.0."""
    g = torch.Generator().manual_seed(5)
    cat, weight = torch.randn(64, 67, generator=g), torch.randn(64, 4, generator=g)
    pre = G.conv_detail(cat, weight, None, 64, False)["pre"]
    windows = [cat[:, k:k + 64] for k in range(4)]
    fused = torch.zeros(64, 64)
    for k in range(4):
        fused = torch.addcmul(fused.double(), weight[:, k:k + 1].double(), windows[k].double()).float()   # one rounding per tap
    newest_first = torch.zeros(64, 64)
    for k in reversed(range(4)):
        newest_first = newest_first + weight[:, k:k + 1] * windows[k]
    assert 0 < int((fused != pre).sum()) and 0 < int((newest_first != pre).sum())
    zero = G.conv_detail(torch.tensor([[0.0, -1.0]]), torch.tensor([[0.0, 0.0]]), None, 1, False)["out"]
    assert same_bits(zero, torch.tensor([[0.0]]))


def test_short_conv_ops_is_a_set_of_its_own():
    assert tuple(mo.SHORT_CONV_OPS) == NAMES and tuple(mo.core.SHORT_CONV_OPS) == NAMES and tuple(mo.core.operators.SHORT_CONV_OPS) == NAMES
    others = (mo.EXTENDED_OPS, mo.KV_INT8_OPS, mo.KV_INT8_SWA_OPS, mo.QUANT_MOE_OPS, mo.SAMPLING_OPS, mo.BEYOND_SURVEY_OPS, mo.NSTEP_OPS,
              mo.NSTEP_KV_INT8_OPS, mo.PACKED_ATTN_OPS, mo.FULL_ATTN_OPS, mo.QUANT_DENSE_OPS, mo.DIT_BLOCK_OPS, mo.VISION_TOWER_OPS,
              mo.EMBEDDING_OPS)
    for name in NAMES:
        assert getattr(mo, name).__name__ == name and getattr(mo.core, name) is getattr(mo, name)
        assert name not in mo.__all__ and name not in mo.core.__all__ and name not in mo.core.operators.__all__
        assert all(name not in other for other in others)
        assert MojoOperator in getattr(mo, name).__bases__


def test_dispatch_registers_torch_and_hip(monkeypatch):
    from mojo_opset_amd.backends import hip
    from mojo_opset_amd.backends.hip import operators

    for name in NAMES:
        core = getattr(mo, name)
        assert core.get_backend_impl("torch", strict=True) is G.GOLDENS[name]
        hip_cls = getattr(hip, "HIP" + name[4:])
        assert getattr(operators, "HIP" + name[4:]) is hip_cls
        assert issubclass(hip_cls, core) and hip_cls.supported_platforms_list == ["rocm"]
        assert hip_cls.__module__.endswith("operators.convolution")
        if get_platform() == "rocm":
            assert core.get_backend_impl("hip", strict=True) is hip_cls
            monkeypatch.setenv("MOJO_BACKEND", "hip")
            assert type(core()) is hip_cls


def test_rebase_registers_the_classes_the_reference_has():
    """The reference has `MojoCausalConv1dUpdateState` and no operator class `MojoCausalConv1d`: the plugin re-bases the first and
    skips the second, as it does for every op this repository defines on its own."""
    from mojo_opset_amd import plugin
    from mojo_opset_amd.backends import hip

    ref = types.ModuleType("stand_in_short_conv_reference")
    core = type(NAMES[0], (MojoOperator,), {"__init__": lambda self, *a, **k: MojoOperator.__init__(self),
                                            "forward": lambda self, *a, **k: None, "__module__": ref.__name__})
    setattr(ref, NAMES[0], core)
    sys.modules[ref.__name__] = ref
    try:
        made = plugin.rebase_hip_backend(ref, platforms=["rocm", "cpu"])
    finally:
        del sys.modules[ref.__name__]
    assert set(made) == {NAMES[0]}
    cls = made[NAMES[0]]
    assert cls.__name__ == "HIPCausalConv1dUpdateState" and issubclass(cls, core) and cls.forward is hip.HIPCausalConv1dUpdateState.forward


def test_contract_errors_need_no_gpu():
    from mojo_opset_amd.backends import hip
    from mojo_opset_amd.backends.hip.lib import MojoHipError

    hidden, state = torch.zeros(2, 8, 5), torch.zeros(2, 8, 4)
    x = torch.zeros(2, 5, 8)
    for update, conv in ((hip.HIPCausalConv1dUpdateState(), hip.HIPCausalConv1d()), (G.TorchCausalConv1dUpdateState(), G.TorchCausalConv1d())):
        with pytest.raises(NotImplementedError, match="width 5"):
            update.forward(hidden, state, torch.zeros(8, 5))
        with pytest.raises(NotImplementedError, match="width 5"):
            conv.forward(x, torch.zeros(8, 5))
        with pytest.raises(NotImplementedError, match="width 1"):
            conv.forward(x, torch.zeros(8, 1))
        with pytest.raises(NotImplementedError, match="shorter than width - 1 = 3"):
            update.forward(hidden, state[..., :2], torch.zeros(8, 4))
        with pytest.raises(NotImplementedError, match="up to 8"):
            update.forward(hidden, torch.zeros(2, 8, 9), torch.zeros(8, 4))
        for mixed in (dict(hidden_states=hidden.half()), dict(conv_state=state.bfloat16()), dict(weight=torch.zeros(8, 4).half()),
                      dict(bias=torch.zeros(8).half())):
            kw = dict(dict(hidden_states=hidden, conv_state=state, weight=torch.zeros(8, 4), bias=None), **mixed)
            with pytest.raises(NotImplementedError, match="share one dtype"):
                update.forward(**kw)
        for mixed in (dict(bias=torch.zeros(8).half()), dict(residual=x.half()), dict(initial_state=torch.zeros(2, 8, 3).bfloat16())):
            with pytest.raises(NotImplementedError, match="share one dtype"):
                conv.forward(x, torch.zeros(8, 4), **mixed)
        with pytest.raises(NotImplementedError, match="float64"):
            conv.forward(x.double(), torch.zeros(8, 4).double())
        for act in ("gelu", "relu", ""):
            with pytest.raises(NotImplementedError, match="activation"):
                update.forward(hidden, state, torch.zeros(8, 4), None, act)
            with pytest.raises(NotImplementedError, match="activation"):
                conv.forward(x, torch.zeros(8, 4), activation=act)
        with pytest.raises(NotImplementedError, match="int32 or int64"):
            conv.forward(x[:1], torch.zeros(8, 4), cu_seqlens=torch.tensor([0.0, 5.0]))
        with pytest.raises(ValueError, match="packed"):
            conv.forward(x, torch.zeros(8, 4), cu_seqlens=torch.tensor([0, 5]))
        with pytest.raises(ValueError, match="initial_state must be"):
            conv.forward(x, torch.zeros(8, 4), initial_state=torch.zeros(2, 8, 4))
        with pytest.raises(ValueError, match="residual"):
            conv.forward(x, torch.zeros(8, 4), residual=x[:, :4])
    with pytest.raises(MojoHipError, match="CPU tensor"):                  # inside the envelope: the device check is next
        hip.HIPCausalConv1dUpdateState().forward(hidden, state, torch.zeros(8, 4))
    with pytest.raises(MojoHipError, match="CPU tensor"):
        hip.HIPCausalConv1d().forward(x, torch.zeros(8, 4))
    out, final = hip.HIPCausalConv1d().forward(x[:, :0], torch.zeros(8, 4), initial_state=torch.ones(2, 8, 3), output_final_state=True)
    assert out.shape == (2, 0, 8) and bool((final == 1).all())             # no token: no device call, the state passes through


def test_header_and_binding_agree_on_the_entry_points():
    from mojo_opset_amd.backends.hip import lib as L

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mojo_hip.h")).read(), flags=re.S)
    kinds = {"const void*": L.c_void_p, "void*": L.c_void_p, "mojo_stream_t": L.c_void_p, "int64_t": L.c_int64, "int": L.c_int}
    found = re.search(r"\bint\s+" + ENTRY_POINT + r"\s*\(([^)]*)\)\s*;", header)
    assert found and ENTRY_POINT in L.SIGNATURES
    declared = [kinds[" ".join(p.split()[:-1])] for p in found.group(1).split(",")]
    restype, argtypes = L.SIGNATURES[ENTRY_POINT]
    assert restype is L.c_int and list(argtypes) == declared
    for name in ("mojo_hip_causal_conv1d_run_tokens", "mojo_hip_causal_conv1d_row_thread_max_t"):
        assert re.search(r"\bint64_t\s+" + name + r"\s*\(\s*void\s*\)\s*;", header) and L.SIGNATURES[name] == (L.c_int64, [])
    text = open(os.path.join(ROOT, "mojo_opset_amd", "csrc", "causal_conv1d.hip")).read()
    assert set(re.findall(r"MOJO_HIP_[A-Z0-9_]+", text)) == set()                                           # no switch of its own
    assert re.search(r'extern "C" int ' + ENTRY_POINT + r"\(", text)
    assert "__fmul_rn" in text and "__fadd_rn" in text and "activation_math.h" in text
    lib = L.load()
    assert lib.mojo_hip_causal_conv1d_run_tokens() >= 3 and lib.mojo_hip_causal_conv1d_row_thread_max_t() >= 8


def test_a_state_view_whose_rows_overlap_is_not_updated_in_place():
    """One thread owns one row of the in-place update, so the kernel addresses only states whose rows are disjoint."""
    from mojo_opset_amd.backends.hip.operators.convolution import _state_rows

    base = torch.zeros(2 * 8 * 4 + 64)
    assert _state_rows(base[:64].view(2, 8, 4)) and _state_rows(torch.zeros(2, 8, 6)[:, :, :4])
    assert _state_rows(torch.zeros(8, 2, 4).transpose(0, 1)) and _state_rows(torch.zeros(1, 8, 4)) and _state_rows(torch.zeros(2, 1, 4))
    assert not _state_rows(base.as_strided((2, 8, 4), (4, 4, 1)))            # equal strides: row (1, 0) is row (0, 1)
    assert not _state_rows(base.as_strided((2, 8, 4), (16, 4, 1)))           # a sequence starts inside the previous one
    assert not _state_rows(base.as_strided((2, 8, 4), (32, 2, 1)))           # rows closer than a row
    assert not _state_rows(torch.zeros(2, 4, 8).transpose(1, 2))             # columns not dense
