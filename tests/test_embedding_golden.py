"""The input-embedding ops (`EMBEDDING_OPS`: the plain and the vocabulary-parallel embedding, the over-encoding layer with its
n-gram ids, the packed-NF4 lookup) without a GPU: the goldens against the recorded reference outputs, the set and its wiring,
dispatch and the plugin, constructors, `extra_repr` and `state_dict` keys, the contract errors of the `HIP<Op>.forward`s (reached
before any device call), the C header, and a scalar restatement of the n-gram recurrence.

The recorded outputs (tests/make_embedding_golden.py) are one file under 256 KiB."""
import os
import re
import sys
import types

import pytest
import torch

import embedding_golden as G
import mojo_opset_amd as mo
from conftest import GOLDEN, ROOT, bit_equal, build_op, clone_tree, load_golden
from hip_utils import max_ulp_bf16ish
from mojo_opset_amd.core import MojoOperator
from mojo_opset_amd.core.operators import over_encoding as OE
from mojo_opset_amd.core.platform import get_platform

NAMES = ("MojoEmbedding", "MojoParallelEmbedding", "MojoOverEncodingNGram", "MojoOverEncoding", "MojoNF4DequantEmbedding")
ENTRY_POINTS = ("mojo_hip_embedding", "mojo_hip_nf4_embedding", "mojo_hip_oe_ngram", "mojo_hip_over_encoding_concat")
CASES = load_golden("embedding")
IDS = [pytest.param(c, id=f"{i}-{c['op']}-{c['label']}") for i, c in enumerate(CASES)]
NGRAM = [c for c in CASES if c["op"] == "MojoOverEncodingNGram"]


@pytest.mark.parametrize("case", IDS)
def test_golden_reproduces_the_reference_bit_for_bit(case):
    op = build_op(G.GOLDENS[case["op"]], case)
    with torch.no_grad():
        out = op.forward(*clone_tree(case["args"]))
    if case["op"] == "MojoOverEncoding":
        # integers and copies up to the concatenation: bit for bit.  The product is a CPU GEMM, whose fp32 summation order belongs
        # to the host: `MojoGemm`'s bound (tests/test_hip_dense.py)
        assert bit_equal(op.concat(*clone_tree(case["args"])), case["concat"])
        with torch.no_grad():
            assert bit_equal(out, op.oe_up_proj(case["concat"]))           # exact on any host: forward is up_proj of that
        assert out.dtype == case["out"].dtype and out.shape == case["out"].shape
        if out.dtype == torch.float32:
            torch.testing.assert_close(out, case["out"], atol=1e-4, rtol=1e-4)
        else:
            assert max_ulp_bf16ish(out, case["out"], atol=2e-3) <= 1
        return
    assert bit_equal(out, case["out"])                                       # (dtypes included: bit_equal compares them)


@pytest.mark.parametrize("case", IDS)
def test_constructor_repr_and_state_dict_keys_follow_the_recording(case):
    from mojo_opset_amd.backends import hip

    for cls in (G.GOLDENS[case["op"]], getattr(hip, "HIP" + case["op"][4:])):
        op = build_op(cls, case)
        assert op.extra_repr() == case["repr"]
        assert list(op.state_dict().keys()) == case["state_keys"]
        for key, value in case["state"].items():
            assert op.state_dict()[key].dtype == value.dtype and op.state_dict()[key].shape == value.shape


def test_fixture_is_small_and_covers_the_cases():
    assert os.path.getsize(os.path.join(GOLDEN, "embedding.pt")) < 256 * 1024
    assert {c["op"] for c in CASES} == set(NAMES)
    labels = {c["label"]: c for c in NGRAM}
    for label in ("one-to-five", "257-ragged-5-7-9", "257-ragged-8-9-11", "97-ragged-4-6", "193-ragged-3-5-7", "decode-b48-s1",
                  "perf-prefill-2x64", "perf-decode-128x1"):
        assert label in labels
    assert any(c["args"][0].dim() == 2 and c["args"][0].shape[1] > 1 for c in NGRAM)                       # [B, S > 1]
    assert any(c["args"][1].shape[1] > max(c["ctor"]["kwargs"]["oe_grams"]) - 1 for c in NGRAM)             # a longer history
    one = labels["gram-1-id-above-v"]
    assert one["ctor"]["kwargs"]["oe_grams"][0] == 1 and int(one["out"][0, 0]) == 50 > one["ctor"]["kwargs"]["oe_vocab_sizes"][0]
    big = labels["two-to-the-31"]
    assert int(big["out"].max()) > 2 ** 32 and big["ctor"]["kwargs"]["ori_vocab_size"] == 2 ** 31 - 1
    i32 = labels["int32"]
    assert i32["args"][0].dtype == torch.int32 and i32["out"].dtype == torch.int32                          # int32 in, int32 out
    nf4 = [c for c in CASES if c["op"] == "MojoNF4DequantEmbedding"]
    assert {c["ctor"]["kwargs"]["group_size"] for c in nf4} >= {1, 3, 64}
    assert {c["ctor"]["args"][0].dtype for c in nf4} == {torch.int8, torch.uint8}
    assert {c["ctor"]["kwargs"]["output_dtype"] for c in nf4} == {torch.float32, torch.bfloat16, torch.float16}
    for c in nf4:
        start, rows, ids = c["ctor"]["kwargs"]["vocab_start_id"], c["ctor"]["args"][0].shape[0], c["args"][0]
        if start:
            assert bool((ids < start).any()) and bool((ids >= start + rows).any()) and bool(((ids >= start) & (ids < start + rows)).any())
    assert any(c["args"][0].numel() == 0 for c in nf4)
    layers = [c for c in CASES if c["op"] == "MojoOverEncoding"]
    assert {"_mega_embedding_scale" in c["ctor"]["kwargs"] for c in layers} == {True, False}                 # NF4 and dense
    assert {len(c["args"]) for c in layers} == {2, 3}                                                        # batched and packed


def test_the_one_to_five_table_of_the_reference():
    case = next(c for c in NGRAM if c["label"] == "one-to-five")
    offsets = torch.arange(6) * 10 ** 4
    assert torch.equal(case["out"] - offsets, case["expected_at_offset_0"])
    assert case["expected_at_offset_0"][4].tolist() == [45, 45, 345, 345, 2345, 2345]


@pytest.mark.parametrize("case", [pytest.param(c, id=c["label"]) for c in NGRAM])
def test_a_scalar_restatement_of_the_recurrence_equals_the_golden(case):
    """Python integers, token by token: exact at any size (the 2^31 case needs 63 bits)."""
    kw = case["ctor"]["kwargs"]
    sizes = kw["oe_vocab_sizes"]
    offsets = [sum(sizes[:g]) for g in range(len(sizes))]
    ids, hist = case["args"][0], case["args"][1]
    if len(case["args"]) == 3:
        rows, start = [], 0
        for b, n in enumerate(case["args"][2].tolist()):
            rows += G.ngram_ids_scalar(ids[start:start + n].tolist(), hist[b].tolist(), sizes, offsets, kw["oe_grams"], kw["ori_vocab_size"])
            start += n
        assert rows == case["out"].tolist()
    else:
        rows = [G.ngram_ids_scalar(ids[b].tolist(), hist[b].tolist(), sizes, offsets, kw["oe_grams"], kw["ori_vocab_size"])
                for b in range(ids.shape[0])]
        assert rows == case["out"].tolist()


def test_nf4_traps_show_on_random_rows():
    """64 x 256 random rows against the golden: an fp32 codebook or a fused multiply-add changes thousands of fp32 outputs."""
    g = torch.Generator().manual_seed(7)
    nib = torch.randint(0, 16, (64, 256), generator=g, dtype=torch.uint8)
    packed = nib[:, 0::2] | (nib[:, 1::2] << 4)
    scale, mean = torch.randn(64, 4, generator=g), torch.randn(64, 4, generator=g)
    book16 = OE.get_nf4_codebook("cpu")
    want = G.dequantize_nf4(packed, scale, mean, 64, book16, torch.float32)
    assert torch.equal(G.unpack_nf4(packed), nib.long())
    s, m = scale.repeat_interleave(64, 1), mean.repeat_interleave(64, 1)
    book32 = torch.tensor(OE.NF4_CODEBOOK, dtype=torch.float32)
    assert int((book32[nib.long()] * s + m != want).sum()) > 8000
    fused = (book16.double()[nib.long()] * s.double() + m.double()).float()                               # one rounding
    assert 500 < int((fused != want).sum()) < 6000
    assert torch.equal(book16.float()[nib.long()] * s + m, want)


def test_embedding_ops_is_a_set_of_its_own():
    assert tuple(mo.EMBEDDING_OPS) == NAMES and tuple(mo.core.EMBEDDING_OPS) == NAMES and tuple(mo.core.operators.EMBEDDING_OPS) == NAMES
    others = (mo.EXTENDED_OPS, mo.KV_INT8_OPS, mo.KV_INT8_SWA_OPS, mo.QUANT_MOE_OPS, mo.SAMPLING_OPS, mo.BEYOND_SURVEY_OPS, mo.NSTEP_OPS,
              mo.NSTEP_KV_INT8_OPS, mo.PACKED_ATTN_OPS, mo.FULL_ATTN_OPS, mo.QUANT_DENSE_OPS, mo.DIT_BLOCK_OPS, mo.VISION_TOWER_OPS)
    for name in NAMES:
        assert getattr(mo, name).__name__ == name and getattr(mo.core, name) is getattr(mo, name)
        assert name not in mo.__all__ and name not in mo.core.__all__ and name not in mo.core.operators.__all__
        assert all(name not in other for other in others)
        assert MojoOperator in getattr(mo, name).__bases__


def test_dispatch_registers_torch_and_hip():
    from mojo_opset_amd.backends import hip

    for name in NAMES:
        core = getattr(mo, name)
        assert core.get_backend_impl("torch", strict=True) is G.GOLDENS[name]
        hip_cls = getattr(hip, "HIP" + name[4:])
        assert issubclass(hip_cls, core) and hip_cls.supported_platforms_list == ["rocm"]
        assert hip_cls.__module__.endswith("operators.embedding")
        if get_platform() == "rocm":
            assert core.get_backend_impl("hip", strict=True) is hip_cls
    from mojo_opset_amd.backends.hip.operators import embedding as backend

    assert callable(backend.over_encoding_concat)                          # the fused launch, exposed as `dense_gemm_swiglu` is


def test_rebase_registers_the_classes_the_reference_has():
    from mojo_opset_amd import plugin
    from mojo_opset_amd.backends import hip

    ref = types.ModuleType("stand_in_embedding_reference")

    def make(name):
        core = type(name, (MojoOperator,), {"__init__": lambda self, *a, **k: MojoOperator.__init__(self),
                                            "forward": lambda self, *a, **k: None, "__module__": ref.__name__})
        setattr(ref, name, core)
        return core

    cores = {name: make(name) for name in NAMES}
    sys.modules[ref.__name__] = ref
    try:
        made = plugin.rebase_hip_backend(ref, platforms=["rocm", "cpu"])
    finally:
        del sys.modules[ref.__name__]
    for name, core in cores.items():
        cls, mine = made[name], getattr(hip, "HIP" + name[4:])
        assert cls.__name__ == mine.__name__ and issubclass(cls, core)
        assert cls.forward is mine.forward and "__init__" not in vars(cls)


def test_the_layer_builds_the_nf4_table_of_its_own_backend_and_loads_without_the_workspace_buffers():
    from mojo_opset_amd.backends import hip

    case = next(c for c in CASES if c["label"] == "nf4-g1-packed")
    for cls, nf4_cls in ((G.TorchOverEncoding, G.TorchNF4DequantEmbedding), (hip.HIPOverEncoding, hip.HIPNF4DequantEmbedding)):
        op = build_op(cls, case)
        assert type(op.oe_mega_embedding) is nf4_cls and op.oe_mega_embedding.codebook.dtype == torch.float16
        assert torch.equal(op.oe_vocab_offsets, torch.tensor([0, 23, 52, 83])) and op.oe_vocab_offsets.dtype == torch.int64
        state = {k: v for k, v in op.state_dict().items() if k not in OE.WORKSPACE_BUFFERS}
        assert len(state) == len(op.state_dict()) - 3
        result = op.load_state_dict(state, strict=True)                       # the hook drops the three derived buffers
        assert result.missing_keys == [] and result.unexpected_keys == []
        with pytest.raises(RuntimeError, match="oe_up_proj.weight"):
            op.load_state_dict({k: v for k, v in state.items() if k != "oe_up_proj.weight"}, strict=True)
    dense = build_op(hip.HIPOverEncoding, next(c for c in CASES if c["label"] == "dense-fp32-packed"))
    assert type(dense.oe_mega_embedding) is torch.nn.Embedding and dense.oe_mega_embedding.weight.shape == (120, 8)
    ngram = hip.HIPOverEncodingNGram(10, [7, 9], [2, 3])
    assert ngram.state_dict() == {} and ngram.oe_vocab_offsets.tolist() == [0, 7] and ngram.oe_grams.dtype == torch.int64
    par = hip.HIPParallelEmbedding(257, 4, padding_idx=2)
    assert (par.vocab_start_index, par.vocab_end_index, par.local_num_embeddings) == (0, 257, 257) and not par.weight[2].any()


def test_constructor_and_contract_errors_need_no_gpu():
    from mojo_opset_amd.backends import hip
    from mojo_opset_amd.backends.hip.lib import MojoHipError

    ids = torch.tensor([1, 2])
    # ---- the plain lookups
    with pytest.raises(NotImplementedError, match="max_norm"):
        hip.HIPEmbedding(5, 2, max_norm=1.0).forward(ids)
    with pytest.raises(NotImplementedError, match="max_norm"):
        hip.HIPParallelEmbedding(5, 2, max_norm=1.0).forward(ids)
    with pytest.raises(NotImplementedError, match="int32 or int64"):
        hip.HIPEmbedding(5, 2).forward(ids.float())
    with pytest.raises(NotImplementedError, match="float64"):
        hip.HIPEmbedding(5, 2, dtype=torch.float64).forward(ids)
    for op in (hip.HIPEmbedding(5, 2, padding_idx=1), hip.HIPParallelEmbedding(5, 2)):
        with pytest.raises(MojoHipError, match="CPU tensor"):                # inside the envelope: the device check is next
            op.forward(ids)
    # ---- NF4
    q, s = torch.zeros(4, 3, dtype=torch.int8), torch.zeros(4, 2)
    for cls in (hip.HIPNF4DequantEmbedding, G.TorchNF4DequantEmbedding):
        with pytest.raises(ValueError, match="2D"):
            cls(q[0], s, s, group_size=3)
        with pytest.raises(ValueError, match="same shape"):
            cls(q, s, s[:, :1], group_size=3)
        with pytest.raises(ValueError, match="group_size"):
            cls(q, s, s, group_size=0)
        with pytest.raises(ValueError, match="incompatible"):
            cls(q, s, s, group_size=4)
    with pytest.raises(NotImplementedError, match="cpu_only"):
        hip.HIPNF4DequantEmbedding(q, s, s, group_size=3, cpu_only=True)
    nf4 = hip.HIPNF4DequantEmbedding(q, s, s, group_size=3)
    assert nf4.embedding_dim == 6 and nf4.output_dtype == torch.bfloat16 and set(nf4.state_dict()) == {"weight", "scale", "mean", "codebook"}
    assert torch.equal(nf4.codebook, torch.tensor(OE.NF4_CODEBOOK).half())
    empty = nf4.forward(torch.zeros(0, 3, dtype=torch.int64))                 # no device call for an empty input
    assert empty.shape == (0, 3, 6) and empty.dtype == torch.bfloat16
    with pytest.raises(NotImplementedError, match="int32 or int64"):
        nf4.forward(ids.float())
    with pytest.raises(ValueError, match="int8 or uint8"):
        hip.HIPNF4DequantEmbedding(q.short(), s, s, group_size=3).forward(ids)
    with pytest.raises(NotImplementedError, match="output_dtype"):
        hip.HIPNF4DequantEmbedding(q, s, s, group_size=3, output_dtype=torch.float64).forward(ids)
    with pytest.raises(MojoHipError, match="CPU tensor"):
        nf4.forward(ids)
    # ---- the n-gram ids and the layer: the same call contract
    ngram = hip.HIPOverEncodingNGram(10, [7, 9], [2, 4])
    layer = hip.HIPOverEncoding(10, 8, 4, [7, 9], [2, 4])
    hist = torch.zeros(2, 3, dtype=torch.int64)
    for op in (ngram, layer, G.TorchOverEncodingNGram(10, [7, 9], [2, 4])):
        with pytest.raises(ValueError, match="fewer than max gram - 1 = 3"):
            op.forward(torch.tensor([[1], [2]]), hist[:, :2])
        with pytest.raises(AssertionError, match="packed form"):
            op.forward(torch.tensor([[1], [2]]), hist, torch.tensor([1, 1]))
        with pytest.raises(AssertionError, match="packed form"):
            op.forward(ids, hist, torch.tensor([2]))
        with pytest.raises(AssertionError, match="batched form"):
            op.forward(ids, hist)
    for op in (ngram, layer):
        with pytest.raises(NotImplementedError, match="int32 or int64"):
            op.forward(torch.tensor([[1.0], [2.0]]), hist)
        with pytest.raises(MojoHipError, match="CPU tensor"):
            op.forward(torch.tensor([[1], [2]]), hist)
    floats = hip.HIPOverEncodingNGram(10, [7, 9], [2, 4])
    floats.oe_vocab_sizes = floats.oe_vocab_sizes.float()
    with pytest.raises(NotImplementedError, match="oe_vocab_sizes must be int32 or int64"):
        floats.forward(torch.tensor([[1], [2]]), hist)
    with pytest.raises(NotImplementedError, match="mega_embedding_cpu_only"):
        hip.HIPOverEncoding(10, 8, 4, [7, 9], [2, 4], _mega_embedding_weight=torch.zeros(16, 4),
                            mega_embedding_cpu_only=True).forward(torch.tensor([[1], [2]]), hist)
    with pytest.raises(NotImplementedError, match="share one dtype"):
        mixed = hip.HIPOverEncoding(10, 8, 4, [7, 9], [2, 4])
        mixed.oe_up_proj.to(torch.bfloat16)
        mixed.forward(torch.tensor([[1], [2]]), hist)
    with pytest.raises(NotImplementedError, match="float64"):
        hip.HIPOverEncoding(10, 8, 4, [7, 9], [2, 4]).double().forward(torch.tensor([[1], [2]]), hist)


def test_header_and_binding_agree_on_the_entry_points():
    from mojo_opset_amd.backends.hip import lib as L

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mojo_hip.h")).read(), flags=re.S)
    kinds = {"const void*": L.c_void_p, "void*": L.c_void_p, "mojo_stream_t": L.c_void_p, "int64_t": L.c_int64, "int": L.c_int}
    for name in ENTRY_POINTS:
        found = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert found and name in L.SIGNATURES
        declared = [kinds[" ".join(p.split()[:-1])] for p in found.group(1).split(",")]
        restype, argtypes = L.SIGNATURES[name]
        assert restype is L.c_int and list(argtypes) == declared, name
    text = open(os.path.join(ROOT, "mojo_opset_amd", "csrc", "embedding.hip")).read()
    assert set(re.findall(r"MOJO_HIP_[A-Z0-9_]+", text)) == set()                                           # no switch of its own
    for name in ENTRY_POINTS:
        assert re.search(r'extern "C" int ' + name + r"\(", text)
    assert hasattr(L.load(), "mojo_hip_over_encoding_concat")


def test_the_largest_gram_follows_the_buffer():
    """The host keeps the largest gram while `oe_grams` is unchanged; an in-place write (what `load_state_dict` does) or a new
    tensor makes it be read again, so the history check never uses a stale value."""
    from mojo_opset_amd.backends import hip
    from mojo_opset_amd.backends.hip.operators.embedding import _max_gram

    layer = hip.HIPOverEncoding(10, 8, 4, [7, 9], [2, 3])
    ids, hist = torch.tensor([[1], [2]]), torch.zeros(2, 2, dtype=torch.int64)
    assert _max_gram(layer) == 3 and _max_gram(layer) == 3
    state = layer.state_dict()
    state["oe_grams"] = torch.tensor([2, 5])
    layer.load_state_dict(state)
    assert _max_gram(layer) == 5
    with pytest.raises(ValueError, match="fewer than max gram - 1 = 4"):
        layer.forward(ids, hist)
    layer.oe_grams = torch.tensor([6, 2])
    assert _max_gram(layer) == 6
    ngram = hip.HIPOverEncodingNGram(10, [7, 9], [2, 4])
    assert _max_gram(ngram) == 4
    ngram.oe_grams[0] = 7
    assert _max_gram(ngram) == 7
