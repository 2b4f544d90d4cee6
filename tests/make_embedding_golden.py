"""Write tests/golden/embedding.pt: reference outputs of the input-embedding ops (authoring machine only; pytest does not collect
this file).

Usage: python tests/make_embedding_golden.py <reference root>   (or MOJO_REFERENCE_ROOT; nothing else reads it)

The outputs come from the reference's own classes, constructed and called on CPU: `mojo_opset/core/operators/embedding.py`
MojoEmbedding and MojoParallelEmbedding, `core/operators/over_encoding.py` MojoOverEncodingNGram, MojoOverEncoding and
MojoNF4DequantEmbedding.  Each case records the constructor arguments, the instance's ``state_dict()``, the inputs, the output, the
``extra_repr()`` and the ``state_dict`` keys (for the layer also the concatenation its up projection reads) -- tensors, scalars
and strings only; tests/test_embedding_golden.py pins
tests/embedding_golden.py to them bit for bit.  The n-gram cases are those of the reference's accuracy test that carry fixed
numbers (tests/accuracy/operators/test_over_encoding.py) and the ones this repository adds; the layers are small (the file stays
under 256 KiB): the GPU tests compute their goldens from the pinned classes at the shapes they need.
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BF16, F16, F32, I32, I64 = torch.bfloat16, torch.float16, torch.float32, torch.int32, torch.int64

V257 = dict(ori_vocab_size=257, oe_vocab_sizes=[263, 269, 271, 277, 281, 283, 293, 307], oe_grams=[2, 2, 3, 3, 4, 4, 5, 5])
PERF = dict(ori_vocab_size=10086, oe_vocab_sizes=[10086 + 2 ** i for i in range(12)], oe_grams=[i for i in range(2, 8) for _ in range(2)])
PRIMES21 = [11, 13, 15, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67, 71, 73, 79, 83, 89]
HIST257 = [[3, 5, 7, 9], [2, 4, 6, 8], [11, 13, 17, 19]]
BIG = 2 ** 31


def t(values, dtype=I64):
    return torch.tensor(values, dtype=dtype)


def stride3(total, vocab):
    return (torch.arange(1, total + 1, dtype=I64) * 3) % vocab


def ngram_cases():
    """(label, constructor keywords, input_ids, history, q_lens, expected table or None)"""
    basic = dict(ori_vocab_size=10, oe_vocab_sizes=[10 ** 4] * 6, oe_grams=[2, 2, 3, 3, 4, 4])
    long_hist = torch.cat((torch.ones(5, 16, dtype=I64), torch.zeros(5, 3, dtype=I64)), dim=-1)
    expected = t([[1] * 6, [12] * 6, [23, 23, 123, 123, 123, 123], [34, 34, 234, 234, 1234, 1234], [45, 45, 345, 345, 2345, 2345]])
    one_to_five = t([1, 2, 3, 4, 5])
    rows123 = torch.stack([torch.arange(1, 4) for _ in range(5)], dim=0)
    g = torch.Generator().manual_seed(2041)
    big = dict(ori_vocab_size=BIG - 1, oe_vocab_sizes=[BIG + 1, BIG + 11, BIG + 3], oe_grams=[2, 3, 4])
    return [
        ("one-to-five", basic, one_to_five, long_hist[:1], t([5]), expected),             # a history longer than needed, too
        ("one-to-five-batched", basic, one_to_five.unsqueeze(-1), rows123, None, None),
        ("one-to-five-batched-long-history", basic, one_to_five.unsqueeze(-1),
         torch.cat((torch.ones(5, 16, dtype=I64), rows123), dim=1), None, None),
        ("257-ragged-5-7-9", V257, t(PRIMES21), t(HIST257), t([5, 7, 9]), None),
        ("257-ragged-8-9-11", V257, stride3(28, 257), t(HIST257), t([8, 9, 11]), None),
        ("97-ragged-4-6", dict(ori_vocab_size=97, oe_vocab_sizes=[101, 103, 107, 109], oe_grams=[2, 2, 3, 3]), stride3(10, 97),
         t([[5, 7], [11, 13]]), t([4, 6]), None),
        ("193-ragged-3-5-7", dict(ori_vocab_size=193, oe_vocab_sizes=[197, 199, 211, 223, 227, 229], oe_grams=[2, 2, 3, 3, 4, 4]),
         stride3(15, 193), t([[2, 3, 5], [7, 11, 13], [17, 19, 23]]), t([3, 5, 7]), None),
        ("decode-b48-s1", V257, (torch.arange(1, 49, dtype=I64) % 257).view(48, 1), torch.arange(48 * 4, dtype=I64).view(48, 4) % 17,
         None, None),
        ("batched-b3-s6", V257, torch.randint(0, 257, (3, 6), generator=g), torch.randint(0, 257, (3, 7), generator=g), None, None),
        ("gram-1-id-above-v", dict(ori_vocab_size=100, oe_vocab_sizes=[7, 11], oe_grams=[1, 2]), t([50, 3, 99]), t([[4]]), t([3]), None),
        ("two-to-the-31", big, torch.randint(BIG - 1000, BIG - 1, (2, 5), generator=g), torch.randint(BIG - 1000, BIG - 1, (2, 3), generator=g),
         None, None),
        ("int32", dict(ori_vocab_size=97, oe_vocab_sizes=[101, 103, 107, 109], oe_grams=[2, 2, 3, 3]), stride3(10, 97).to(I32),
         t([[5, 7], [11, 13]], I32), t([4, 6], I32), None),
        ("perf-prefill-2x64", PERF, torch.arange(1, 129, dtype=I64), torch.ones(2, 6, dtype=I64), t([64, 64]), None),
        ("perf-decode-128x1", PERF, torch.arange(1, 129, dtype=I64).view(128, 1), torch.ones(128, 6, dtype=I64), None, None),
    ]


def nf4_table(g, rows, dim, group_size, storage=torch.int8, sm_dtype=F32):
    nibbles = torch.randint(0, 16, (rows, dim), generator=g, dtype=torch.uint8)
    packed = (nibbles[:, 0::2] | (nibbles[:, 1::2] << 4))
    packed = packed.view(torch.int8) if storage == torch.int8 else packed
    return packed, torch.randn(rows, dim // group_size, generator=g).to(sm_dtype), torch.randn(rows, dim // group_size, generator=g).to(sm_dtype)


def record(cls, name, label, ctor_args, ctor_kwargs, args, cast=None, init=None, **extra):
    op = cls(*ctor_args, **ctor_kwargs)
    if cast is not None:
        op = op.to(cast)
    if init is not None:
        init(op)
    state = {k: v.detach().clone() for k, v in op.state_dict().items()}
    recorded = tuple(a.clone() if isinstance(a, torch.Tensor) else a for a in args)
    if hasattr(op, "oe_up_proj"):                 # the layer: what its up projection reads is recorded too (pinned bit for bit;
        op.oe_up_proj.register_forward_pre_hook(lambda module, inputs: extra.update(concat=inputs[0].clone()))   # the product is not)
    with torch.no_grad():
        out = op.forward(*args)
    return {"op": name, "label": label, "ctor": {"args": ctor_args, "kwargs": ctor_kwargs}, "cast": cast, "state": state,
            "args": recorded, "kwargs": {}, "out": out, "repr": op.extra_repr(), "state_keys": list(op.state_dict().keys()), **extra}


def main(reference_root):
    sys.path.insert(0, reference_root)
    from mojo_opset.core.operators import embedding as ref_emb
    from mojo_opset.core.operators import over_encoding as ref_oe

    g = torch.Generator().manual_seed(2040)
    cases = []
    # ---- the plain lookups
    ids23 = torch.tensor([[0, 256, 7], [7, 19, 100]])
    cases.append(record(ref_emb.MojoEmbedding, "MojoEmbedding", "fp32", (257, 8), {}, (ids23,)))
    cases.append(record(ref_emb.MojoEmbedding, "MojoEmbedding", "bf16-padding", (257, 7), {"padding_idx": 3, "dtype": BF16}, (ids23.to(I32),)))
    cases.append(record(ref_emb.MojoEmbedding, "MojoEmbedding", "max-norm-repr", (5, 2), {"max_norm": 1.5}, (torch.tensor([1, 4]),)))
    cases.append(record(ref_emb.MojoParallelEmbedding, "MojoParallelEmbedding", "one-shard", (257, 7), {"padding_idx": 2, "dtype": F16},
                        (ids23,)))
    # ---- the n-gram ids
    for label, ctor, ids, hist, lens, expected in ngram_cases():
        args = (ids, hist) if lens is None else (ids, hist, lens)
        case = record(ref_oe.MojoOverEncodingNGram, "MojoOverEncodingNGram", label, (), dict(ctor), args)
        if expected is not None:
            # the reference's test states the table with every vocabulary at offset 0
            assert torch.equal(case["out"] - torch.arange(len(ctor["oe_grams"])) * ctor["oe_vocab_sizes"][0], expected)
            case["expected_at_offset_0"] = expected
        cases.append(case)
    # ---- the NF4 lookup: group sizes 1, 3 (a byte split between two groups) and 64, int8 and uint8 storage, a vocab_start_id
    #      with ids on both sides of the range, every output dtype, fp32 and 16-bit scale / mean
    for label, rows, dim, gs, storage, sm, out_dtype, start, ids in (
            ("g1-int8-fp32", 12, 6, 1, torch.int8, F32, F32, 0, [[0, 11, 5], [12, -1, 3]]),
            ("g3-uint8-bf16", 12, 6, 3, torch.uint8, F32, BF16, 10, [9, 10, 21, 22, -1, 15]),
            ("g64-int8-fp16", 9, 128, 64, torch.int8, BF16, F16, 10, [9, 10, 18, 19, -1]),
            ("g64-uint8-fp32-f16scale", 9, 128, 64, torch.uint8, F16, F32, 0, [8, 0, 4, 4]),
            ("empty", 4, 6, 2, torch.int8, F32, BF16, 0, [])):
        q, s, m = nf4_table(g, rows, dim, gs, storage, sm)
        cases.append(record(ref_oe.MojoNF4DequantEmbedding, "MojoNF4DequantEmbedding", label, (q, s, m),
                            {"group_size": gs, "vocab_start_id": start, "output_dtype": out_dtype}, (torch.tensor(ids, dtype=I64),)))
    # ---- the layer: dense and NF4 mega tables, packed and batched
    small = dict(ori_vocab_size=19, ori_embed_dim=16, oe_embed_dim=8, oe_vocab_sizes=[23, 29, 31, 37], oe_grams=[2, 2, 3, 1])
    packed = (torch.randint(0, 19, (9,), generator=g), torch.randint(0, 19, (3, 2), generator=g), t([4, 1, 4]))
    batched = (torch.randint(0, 19, (3, 2), generator=g), torch.randint(0, 19, (3, 4), generator=g))

    def init(op):
        with torch.no_grad():
            op.oe_up_proj.weight.copy_(torch.randn(op.oe_up_proj.weight.shape, generator=g) * 0.2)

    for label, cast, args in (("dense-fp32-packed", None, packed), ("dense-bf16-batched", BF16, batched), ("dense-fp16-packed", F16, packed)):
        cases.append(record(ref_oe.MojoOverEncoding, "MojoOverEncoding", label, (), dict(small), args, cast=cast, init=init))
    for label, gs, args in (("nf4-g1-packed", 1, packed), ("nf4-g4-batched", 4, batched)):
        q, s, m = nf4_table(g, sum(small["oe_vocab_sizes"]), 8, gs)
        # (with ``dtype`` given the constructor would build the vocabulary buffers in it: they are passed as int64 tensors)
        kwargs = dict(small, oe_vocab_sizes=t(small["oe_vocab_sizes"]), oe_grams=t(small["oe_grams"]), _ori_embedding_weight=torch.randn(19, 16, generator=g), _mega_embedding_weight=q,
                      _mega_embedding_scale=s, _mega_embedding_mean=m, _mega_embedding_group_size=gs, dtype=F32)
        cases.append(record(ref_oe.MojoOverEncoding, "MojoOverEncoding", label, (), kwargs, args, init=init))
    path = os.path.join(ROOT, "tests", "golden", "embedding.pt")
    torch.save({"cases": cases}, path, _use_new_zipfile_serialization=False)   # (the zip form pads every tensor to 64 bytes)
    print(path, os.path.getsize(path), "bytes,", len(cases), "cases")


if __name__ == "__main__":
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("MOJO_REFERENCE_ROOT")
    if not root:
        sys.exit(__doc__)
    main(root)
