"""GPU tests of the over-encoding layer (`MojoOverEncodingNGram`, `MojoOverEncoding`) through the C ABI.

Everything before the up projection is integer arithmetic and copies (and, for an NF4 mega table, the pinned two-rounding
dequantisation), so the n-gram ids and the concatenation are compared bit for bit with the CPU golden (tests/embedding_golden.py,
pinned to the reference by tests/test_embedding_golden.py).  The layer's output is the existing dense GEMM applied to that
concatenation: bit for bit `dense_gemm` of the golden's concatenation, and the torch golden under the judge and bound that
tests/test_hip_dense.py applies to `MojoGemm` (fp32: 1e-4 / 1e-4; 16-bit: one unit in the last place, differences below 2e-3
counting as none)."""
import sys
import types

import pytest
import torch

import embedding_golden as G
from conftest import bit_equal, load_golden
from hip_utils import DEV, hip_cls, last_launch, launches_of, max_ulp_bf16ish, run_hip_case, to_cpu
from mojo_opset_amd.backends.hip.operators.embedding import over_encoding_concat
from mojo_opset_amd.backends.hip.operators.gemm import dense_gemm
from mojo_opset_amd.core import MojoOperator
from mojo_opset_amd.core.operators import over_encoding as OE

pytestmark = pytest.mark.gpu
BF16, F16, F32, I32, I64 = torch.bfloat16, torch.float16, torch.float32, torch.int32, torch.int64
NGRAM, LAYER = "MojoOverEncodingNGram", "MojoOverEncoding"
CASES = load_golden("embedding")
V257 = dict(ori_vocab_size=257, oe_vocab_sizes=[263, 269, 271, 277, 281, 283, 293, 307], oe_grams=[2, 2, 3, 3, 4, 4, 5, 5])


def on_dev(*tensors):
    return tuple(None if t is None else t.to(DEV) for t in tensors)


@pytest.mark.parametrize("case", [pytest.param(c, id=c["label"]) for c in CASES if c["op"] == NGRAM])
def test_ngram_captured_vectors(case):
    """Every recorded case: the reference's fixed-number cases, [B, S > 1], a longer history, a gram of 1, the 2^31 case (63-bit
    products, outputs past 32 bits), int32 in and out, and the reference's perf shapes."""
    got = run_hip_case(case)
    assert got.dtype == case["out"].dtype and torch.equal(to_cpu(got), case["out"])
    assert last_launch() == ("oe_ngram:packed" if len(case["args"]) == 3 else "oe_ngram:batched")


@pytest.mark.parametrize("idt", [I64, I32], ids=["int64", "int32"])
def test_ngram_random_sweep(idt):
    """Every gram from 1 to 7, ragged q_lens with sequences of length 1 and 0 (the golden, like the reference, accepts an empty
    sequence), a history with extra leading columns, packed and batched, more sequences than one chunk table entry each."""
    g = torch.Generator().manual_seed(5)
    vocab, sizes, grams = 1009, [1013, 1019, 1021, 1031, 1033, 1039, 1049, 2053, 997], [1, 2, 3, 4, 5, 6, 7, 7, 3]
    ref, op = G.TorchOverEncodingNGram(vocab, sizes, grams), hip_cls(NGRAM)(vocab, sizes, grams).to(DEV)
    for lens in ([1, 0, 37, 5, 0, 1, 64, 200, 3], [2] * 300 + [0, 1] * 30):
        q_lens = torch.tensor(lens, dtype=idt)
        ids = torch.randint(0, vocab, (sum(lens),), generator=g).to(idt)
        for extra in (0, 5):
            hist = torch.randint(0, vocab, (len(lens), 6 + extra), generator=g).to(idt)
            want = ref.forward(ids, hist, q_lens)
            got = op.forward(*on_dev(ids, hist, q_lens))
            assert got.dtype == idt and torch.equal(to_cpu(got), want), (len(lens), extra)
    ids = torch.randint(0, vocab, (7, 33), generator=g).to(idt)
    hist = torch.randint(0, vocab, (7, 9), generator=g).to(idt)
    assert torch.equal(to_cpu(op.forward(*on_dev(ids, hist))), ref.forward(ids, hist))
    mixed = op.forward(*on_dev(ids, hist.to(I64 if idt == I32 else I32)))       # ids and history need not share a dtype
    assert mixed.dtype == idt and torch.equal(to_cpu(mixed), ref.forward(ids, hist))
    strided = torch.randint(0, vocab, (7, 20), generator=g).to(idt)             # a column slice of a wider history
    assert torch.equal(to_cpu(op.forward(ids.to(DEV), strided.to(DEV)[:, 3:12])), ref.forward(ids, strided[:, 3:12]))


def make_layers(dtype, ori, oe, nf4, group_size=1, seed=0):
    """(golden on the CPU, HIP on the device) over the same tables: vocabulary 257 with the reference's eight n-gram vocabularies."""
    g = torch.Generator().manual_seed(seed + ori + oe)
    rows = sum(V257["oe_vocab_sizes"])
    kw = dict(V257, ori_embed_dim=ori, oe_embed_dim=oe, _ori_embedding_weight=torch.randn(257, ori, generator=g).to(dtype))
    if nf4:
        nib = torch.randint(0, 16, (rows, oe), generator=g, dtype=torch.uint8)
        kw.update(oe_vocab_sizes=torch.tensor(V257["oe_vocab_sizes"]), oe_grams=torch.tensor(V257["oe_grams"]),
                  _mega_embedding_weight=(nib[:, 0::2] | (nib[:, 1::2] << 4)).view(torch.int8),
                  _mega_embedding_scale=torch.randn(rows, oe // group_size, generator=g),
                  _mega_embedding_mean=torch.randn(rows, oe // group_size, generator=g),
                  _mega_embedding_group_size=group_size, dtype=dtype)
    else:
        kw.update(_mega_embedding_weight=torch.randn(rows, oe, generator=g).to(dtype))
    proj = (torch.randn(ori, ori + 8 * oe, generator=g) * 0.02).to(dtype)
    layers = []
    for cls, dev in ((G.TorchOverEncoding, "cpu"), (hip_cls(LAYER), DEV)):
        layer = cls(**{k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()})
        layer.oe_up_proj.weight = torch.nn.Parameter(proj.clone(), requires_grad=False)
        layers.append(layer.to(dev))
    return layers


def inputs(g, packed):
    if packed:
        lens = [5, 1, 0, 9, 16]
        return torch.randint(0, 257, (sum(lens),), generator=g), torch.randint(0, 257, (len(lens), 6), generator=g), torch.tensor(lens)
    return torch.randint(0, 257, (3, 7), generator=g), torch.randint(0, 257, (3, 4), generator=g), None


def separate_launches(layer, ids, hist, q_lens):
    """(3) -> (1) / (2): the n-gram ids, then one lookup per table, concatenated by torch."""
    ngram = hip_cls(NGRAM)(layer.ori_vocab_size, layer.oe_vocab_sizes.tolist(), layer.oe_grams.tolist()).to(DEV)
    oe_ids = ngram.forward(ids, hist, q_lens)
    ori = hip_cls("MojoEmbedding")(2, 1)
    ori.weight = layer.ori_embedding.weight
    mega = layer.oe_mega_embedding
    if not hasattr(mega, "codebook"):
        mega = hip_cls("MojoEmbedding")(2, 1)
        mega.weight = layer.oe_mega_embedding.weight
    return torch.cat((ori.forward(ids), mega.forward(oe_ids).flatten(-2)), dim=-1)


@pytest.mark.parametrize("packed", [True, False], ids=["packed", "batched"])
@pytest.mark.parametrize("nf4", [False, True], ids=["dense", "nf4"])
@pytest.mark.parametrize("ori,oe", [(128, 21), (640, 80), (1536, 192)])
def test_concat_and_layer(ori, oe, nf4, packed):
    """The fused launch writes the golden's `cat` bit for bit and equals the separate launches; the layer equals `dense_gemm` of the
    golden's concatenation bit for bit and the torch golden under `MojoGemm`'s judge.  (128, 21) takes the scalar path: its
    segments start at odd elements.  An NF4 row holds two elements per byte, so the NF4 layer of that size uses 22."""
    if nf4 and oe % 2:
        oe += 1
    for dtype in (BF16, F32, F16):
        group_size = {21 + 1: 11, 80: 1, 192: 64}[oe] if nf4 else 1
        ref, hip = make_layers(dtype, ori, oe, nf4, group_size)
        ids, hist, q_lens = inputs(torch.Generator().manual_seed(ori), packed)
        want_cat = ref.concat(ids, hist, q_lens)
        dev = on_dev(ids, hist, q_lens)
        got_cat = over_encoding_concat(hip, *dev)
        form = last_launch()
        assert bit_equal(got_cat, want_cat), dtype
        assert form == f"oe_concat:{'nf4' if nf4 else 'dense'}:{'scalar' if oe in (21, 22) else 'vec'}:{'packed' if packed else 'batched'}"
        assert bit_equal(separate_launches(hip, *dev), got_cat)
        # the layer: two launches, the GEMM on exactly that buffer
        history = launches_of(lambda: hip.forward(*dev))
        tags = history.split("|")
        assert tags[0].startswith("oe_concat:") and len(tags) >= 2 and all("gemm" in t for t in tags[1:]), history
        got = hip.forward(*dev)
        assert bit_equal(got, dense_gemm(want_cat.to(DEV), hip.oe_up_proj.weight.detach(), None, trans_weight=False))
        with torch.no_grad():
            want = ref.forward(ids, hist, q_lens)
        got = to_cpu(got)
        assert got.dtype == want.dtype and got.shape == want.shape
        if dtype == F32:
            torch.testing.assert_close(got, want, atol=1e-4, rtol=1e-4)
        else:
            assert max_ulp_bf16ish(got, want, atol=2e-3) <= 1


@pytest.mark.parametrize("case", [pytest.param(c, id=c["label"]) for c in CASES if c["op"] == LAYER])
def test_layer_captured_vectors(case):
    got = to_cpu(run_hip_case(case))
    want = case["out"]
    assert got.dtype == want.dtype and got.shape == want.shape
    if want.dtype == F32:
        torch.testing.assert_close(got, want, atol=1e-4, rtol=1e-4)
    else:
        assert max_ulp_bf16ish(got, want, atol=2e-3) <= 1


def test_out_of_range_ids_give_zero_segments_and_never_fault():
    """A token outside the original table, n-gram ids outside an NF4 table that starts at `vocab_start_id`, tokens past
    sum(q_lens): rows of zeros in their segments, everything else the golden's."""
    ref, hip = make_layers(BF16, 128, 32, nf4=False)
    ids, hist, q_lens = inputs(torch.Generator().manual_seed(1), True)
    want = ref.concat(ids, hist, q_lens)
    bad = ids.clone()
    bad[3], bad[7] = 257, -1
    got = to_cpu(over_encoding_concat(hip, *on_dev(bad, hist, q_lens)))
    assert not got[3, :128].any() and not got[7, :128].any()
    keep = [t for t in range(ids.numel()) if t not in (3, 7)]
    assert bit_equal(got[keep, :128], want[keep, :128])
    short = to_cpu(over_encoding_concat(hip, *on_dev(ids, hist, torch.tensor([5, 1, 0, 9, 2]))))      # 14 tokens without a sequence
    assert bit_equal(short[:17], want[:17]) and not short[17:].any()
    ref, hip = make_layers(BF16, 128, 32, nf4=True, group_size=8)
    hip.oe_mega_embedding.vocab_start_id = ref.oe_mega_embedding.vocab_start_id = 1000
    assert bit_equal(over_encoding_concat(hip, *on_dev(ids, hist, q_lens)), ref.concat(ids, hist, q_lens))
    assert bool((ref.concat(ids, hist, q_lens)[:, 128:160] == 0).all())                                 # vocabulary 0 lies below 1000


def test_layer_through_the_plugin_on_a_stand_in_reference():
    """`plugin.rebase_hip_backend` on a stand-in package whose core classes carry the API classes' constructors: the re-based
    class runs this repository's forward and gives the same bits."""
    from mojo_opset_amd import plugin

    stub = types.ModuleType("stand_in_over_encoding_reference")

    def core_like(name):
        def init(self, *args, **kwargs):                       # the API class's constructor: adopt everything it builds
            MojoOperator.__init__(self)
            self.__dict__.update(hip_cls(name)(*args, **kwargs).__dict__)
        return type(name, (MojoOperator,), {"__init__": init, "forward": lambda self, *a, **k: None, "__module__": stub.__name__})

    for name in ("MojoOverEncoding", "MojoOverEncodingNGram"):
        setattr(stub, name, core_like(name))
    sys.modules[stub.__name__] = stub
    try:
        made = plugin.rebase_hip_backend(stub, platforms=["rocm", "cpu"])
    finally:
        del sys.modules[stub.__name__]
    assert set(made) == {"MojoOverEncoding", "MojoOverEncodingNGram"}
    ref, hip = make_layers(BF16, 640, 80, nf4=False)
    rebased = made["MojoOverEncoding"](**dict(V257, ori_embed_dim=640, oe_embed_dim=80)).to(BF16).to(DEV)
    assert issubclass(made["MojoOverEncoding"], stub.MojoOverEncoding) and not isinstance(rebased, OE.MojoOverEncoding)
    rebased.load_state_dict(hip.state_dict())
    for packed in (True, False):
        dev = on_dev(*inputs(torch.Generator().manual_seed(2), packed))
        assert bit_equal(rebased.forward(*dev), hip.forward(*dev))
    ngram = made["MojoOverEncodingNGram"](**V257).to(DEV)
    dev = on_dev(*inputs(torch.Generator().manual_seed(2), True))
    assert torch.equal(ngram.forward(*dev), hip_cls(NGRAM)(**V257).to(DEV).forward(*dev))


def test_decode_form_is_captured_in_a_graph_and_replayed_on_new_inputs():
    """B 16, S 1: the forward makes no host synchronisation, so it captures; the replay on new ids and history equals the eager
    call."""
    for nf4 in (False, True):
        ref, hip = make_layers(BF16, 640, 80, nf4=nf4, group_size=16)
        g = torch.Generator().manual_seed(9)
        ids, hist = torch.randint(0, 257, (16, 1), generator=g).to(DEV), torch.randint(0, 257, (16, 4), generator=g).to(DEV)
        hip.forward(ids, hist)                                               # (the first call reads the largest gram once)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = hip.forward(ids, hist)
        new_ids, new_hist = torch.randint(0, 257, (16, 1), generator=g), torch.randint(0, 257, (16, 4), generator=g)
        ids.copy_(new_ids)
        hist.copy_(new_hist)
        graph.replay()
        torch.cuda.synchronize()
        eager = hip.forward(new_ids.to(DEV), new_hist.to(DEV))
        assert bit_equal(out, eager)
        with torch.no_grad():
            assert max_ulp_bf16ish(to_cpu(out), ref.forward(new_ids, new_hist), atol=2e-3) <= 1


def test_expanded_and_overlapping_views_are_read_as_the_golden_reads_them():
    """A broadcast history (`row.expand(B, H)`, strides (0, 1)), one whose rows overlap and an expanded table are legal inputs of
    the reference: the ids and the concatenation equal the golden's, as for the dense copies."""
    ref, hip = make_layers(BF16, 128, 32, nf4=False)
    ngram_ref, ngram = G.TorchOverEncodingNGram(**V257), hip_cls(NGRAM)(**V257).to(DEV)
    g = torch.Generator().manual_seed(4)
    row = torch.randint(0, 257, (1, 6), generator=g)
    flat = torch.randint(0, 257, (16,), generator=g)
    for packed in (True, False):
        ids, _, q_lens = inputs(torch.Generator().manual_seed(8), packed)
        batch = 5 if packed else 3
        views = ((row.expand(batch, 6), row.to(DEV).expand(batch, 6)),
                 (flat.as_strided((batch, 6), (2, 1)), flat.to(DEV).as_strided((batch, 6), (2, 1))))
        for hist_cpu, hist_dev in views:
            assert hist_dev.stride(0) < 6
            lens_dev = None if q_lens is None else q_lens.to(DEV)
            assert torch.equal(to_cpu(ngram.forward(ids.to(DEV), hist_dev, lens_dev)), ngram_ref.forward(ids, hist_cpu, q_lens))
            assert bit_equal(over_encoding_concat(hip, ids.to(DEV), hist_dev, lens_dev), ref.concat(ids, hist_cpu, q_lens))
    one = torch.randn(1, 24, generator=g).to(BF16)
    table = hip_cls("MojoEmbedding")(2, 1)
    table.weight = torch.nn.Parameter(one.to(DEV).expand(9, 24), requires_grad=False)
    picks = torch.tensor([0, 8, 9, -1, 3])
    assert bit_equal(table.forward(picks.to(DEV)), G.lookup_rows(one.expand(9, 24), picks))


def test_a_loaded_larger_gram_is_seen_by_the_next_forward():
    """`oe_grams` is a buffer of the layer: after a `load_state_dict` with larger grams the ids follow the new buffer (the host's
    largest gram is read again), and equal the golden's."""
    ref, hip = make_layers(BF16, 128, 32, nf4=False)
    ids, hist, q_lens = inputs(torch.Generator().manual_seed(3), True)
    dev = on_dev(ids, hist, q_lens)
    assert bit_equal(over_encoding_concat(hip, *dev), ref.concat(ids, hist, q_lens))
    grams = torch.tensor([7, 6, 5, 4, 3, 2, 1, 7])
    for layer in (ref, hip):
        state = layer.state_dict()
        state["oe_grams"] = grams.clone()
        layer.load_state_dict(state)
    assert bit_equal(over_encoding_concat(hip, *dev), ref.concat(ids, hist, q_lens))
