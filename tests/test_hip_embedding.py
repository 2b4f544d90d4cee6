"""GPU tests of the row gathers of `EMBEDDING_OPS` (`MojoEmbedding`, `MojoParallelEmbedding`, `MojoNF4DequantEmbedding`) through the
C ABI.  Everything is compared bit for bit with the CPU goldens (tests/embedding_golden.py, pinned to the reference by
tests/test_embedding_golden.py): a gather is a copy, and the NF4 value is two fp32 roundings and one rounding to the output dtype,
which the kernel reproduces (the fp32-output case on 64 x 256 random rows is the one a fused multiply-add or an fp32 codebook
fails)."""
import pytest
import torch

import embedding_golden as G
from conftest import bit_equal, load_golden
from hip_utils import DEV, hip_cls, last_launch, run_hip_case, to_cpu
from mojo_opset_amd.backends.hip import lib as L

pytestmark = pytest.mark.gpu
BF16, F16, F32, I32, I64 = torch.bfloat16, torch.float16, torch.float32, torch.int32, torch.int64
ROWS = 257
CASES = [c for c in load_golden("embedding") if c["op"] in ("MojoEmbedding", "MojoParallelEmbedding", "MojoNF4DequantEmbedding")]


@pytest.mark.parametrize("case", [pytest.param(c, id=f"{c['op']}-{c['label']}") for c in CASES if c["label"] != "max-norm-repr"])
def test_captured_vectors(case):
    assert bit_equal(run_hip_case(case), case["out"])


def embedding(table):
    """A `HIPEmbedding` over ``table`` (a device tensor, used in place: a column slice keeps its row stride)."""
    op = hip_cls("MojoEmbedding")(2, 1, dtype=table.dtype)
    op.num_embeddings, op.embedding_dim = table.shape
    op.weight = torch.nn.Parameter(table, requires_grad=False)
    return op


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("dim", [1, 7, 8, 1536])
def test_gather_is_the_golden_bit_for_bit(dim, dtype):
    """Every id form on one table: int32 / int64, shapes [], [5] and [2, 3], non-contiguous, repeats, and the ids -1 and `rows`,
    which give rows of zeros.  dim 8 and 1536 take 16-byte vectors, 1 and 7 single elements."""
    g = torch.Generator().manual_seed(dim)
    table = torch.randn(ROWS, dim, generator=g).to(dtype)
    op = embedding(table.to(DEV))
    wide = torch.randint(0, ROWS, (2, 6), generator=g)
    forms = [torch.tensor(256), torch.tensor([0, 256, 7, 7, 7]), torch.tensor([[3, -1, 9], [ROWS, 0, 3]]), wide[:, ::2],
             torch.tensor([-1, ROWS, 2 ** 40, -2 ** 62])]
    for ids in forms:
        for idt in (I64, I32):
            if idt == I32 and int(ids.abs().max()) >= 2 ** 31:
                continue
            want = G.lookup_rows(table, ids)
            got = op.forward(ids.to(idt).to(DEV))
            assert bit_equal(got, want), (tuple(ids.shape), idt)
    assert last_launch().startswith("embedding:vec16" if dim * table.element_size() % 16 == 0 else "embedding:scalar")
    zeros = to_cpu(op.forward(torch.tensor([-1, ROWS], device=DEV)))
    assert not zeros.any()


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_gather_reads_a_column_slice_in_place_and_writes_a_slice_of_a_wider_buffer(dtype):
    """The table is a column slice of a wider one: of 45 columns (a row stride that is no multiple of 16 bytes: the scalar path),
    or of 48 columns from column 1 (an unaligned base: scalar) or from column 8 (aligned: vectors).  The output is a column slice
    of a buffer whose other columns hold a sentinel that must survive."""
    g = torch.Generator().manual_seed(3)
    wide45, wide48 = (torch.randn(ROWS, w, generator=g).to(dtype).to(DEV) for w in (45, 48))
    ids = torch.randint(-2, ROWS + 2, (37,), generator=g)
    for wide, first, dim, form in ((wide45, 8, 24, "scalar"), (wide48, 1, 24, "scalar"), (wide48, 8, 24, "vec16"), (wide48, 8, 32, "vec16")):
        table = wide[:, first:first + dim]
        got = embedding(table).forward(ids.to(DEV))
        assert bit_equal(got, G.lookup_rows(table.cpu(), ids)) and last_launch().startswith("embedding:" + form), (first, dim)
        for lead in (16, 3):                                            # an aligned and an unaligned destination
            buf = torch.full((ids.numel(), lead + dim + 8), 7.0, dtype=dtype, device=DEV)
            out = buf[:, lead:lead + dim]
            idev = ids.to(DEV)
            L.check(L.load().mojo_hip_embedding(L.ptr(idev), 1, L.ptr(table), L.ptr(out), ids.numel(), ROWS, dim, 0, table.stride(0),
                                                buf.stride(0), L.dtype_code(dtype), L.stream_of(buf)), "embedding")
            assert bit_equal(out, got)
            assert bool((buf[:, :lead] == 7.0).all()) and bool((buf[:, lead + dim:] == 7.0).all())


def test_parallel_embedding_shards_sum_to_the_full_lookup():
    """A 257-row table cut into shards of 65 (the last one holds 62 rows): the shard outputs summed in fp32 equal the full
    lookup, and every token is non-zero in exactly one shard."""
    g = torch.Generator().manual_seed(11)
    table = (torch.randn(ROWS, 24, generator=g).abs() + 0.5).to(BF16)
    ids = torch.cat([torch.randint(0, ROWS, (3, 40), generator=g), torch.tensor([[0, 64, 65, 129, 130, 194, 195, 256] * 5])])
    total = torch.zeros(*ids.shape, 24)
    owners = torch.zeros(ids.shape, dtype=torch.int64)
    for rank in range(4):
        op = hip_cls("MojoParallelEmbedding")(ROWS, 24, dtype=BF16)
        op.vocab_start_index, op.vocab_end_index = rank * 65, min(rank * 65 + 65, ROWS)
        op.local_num_embeddings = op.vocab_end_index - op.vocab_start_index
        op.weight = torch.nn.Parameter(table[op.vocab_start_index:op.vocab_end_index].to(DEV), requires_grad=False)
        out = to_cpu(op.forward(ids.to(DEV)))
        assert op.local_num_embeddings == (65 if rank < 3 else 62) and f"local_range=[{rank * 65}, " in op.extra_repr()
        total += out.float()
        owners += out.float().abs().sum(-1).ne(0).long()
    assert torch.equal(total, table[ids].float()) and bool((owners == 1).all())


def nf4_table(g, rows, dim, group_size, storage, sm_dtype):
    nib = torch.randint(0, 16, (rows, dim), generator=g, dtype=torch.uint8)
    packed = nib[:, 0::2] | (nib[:, 1::2] << 4)
    packed = packed.view(torch.int8) if storage == torch.int8 else packed
    groups = dim // group_size
    return packed, torch.randn(rows, groups, generator=g).to(sm_dtype), torch.randn(rows, groups, generator=g).to(sm_dtype)


@pytest.mark.parametrize("out_dtype", [F32, BF16, F16], ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("dim", [6, 128, 4096])
def test_nf4_is_the_golden_bit_for_bit(dim, out_dtype):
    """group_size {1, 3, 64, dim} where it divides dim, fp32 and 16-bit scale / mean, int8 and uint8 storage, vocab_start_id 10
    with the ids 9, 10, the last valid id, one past it and -1."""
    rows, start = 40, 10
    ids = torch.tensor([[9, 10, start + rows - 1], [start + rows, -1, 25]])
    for n, gs in enumerate(gs for gs in (1, 3, 64, dim) if dim % gs == 0):
        for sm in (F32, BF16, F16):
            g = torch.Generator().manual_seed(dim + gs)
            q, s, m = nf4_table(g, rows, dim, gs, torch.int8 if n % 2 else torch.uint8, sm)
            kw = dict(group_size=gs, vocab_start_id=start, output_dtype=out_dtype)
            want = G.TorchNF4DequantEmbedding(q, s, m, **kw).forward(ids)
            for idt in (I64, I32):
                got = hip_cls("MojoNF4DequantEmbedding")(q.to(DEV), s.to(DEV), m.to(DEV), **kw).forward(ids.to(idt).to(DEV))
                assert bit_equal(got, want), (gs, sm, idt)
            assert last_launch().startswith("nf4_embedding:vec8" if dim % 8 == 0 else "nf4_embedding:scalar")
            assert not to_cpu(got)[1, :2].any() and not to_cpu(got)[0, 0].any()


def test_nf4_fp32_output_on_random_rows_and_an_empty_input():
    """64 x 256 random rows, fp32 out: 0 differing values.  An fp32 codebook would change about 13 000 of the 16 384 and a fused
    multiply-add about 2 400 (tests/test_embedding_golden.py counts both on the CPU)."""
    g = torch.Generator().manual_seed(7)
    for gs in (64, 1):
        q, s, m = nf4_table(g, 64, 256, gs, torch.int8, F32)
        op = hip_cls("MojoNF4DequantEmbedding")(q.to(DEV), s.to(DEV), m.to(DEV), group_size=gs, output_dtype=F32)
        ids = torch.randperm(64, generator=g)
        want = G.TorchNF4DequantEmbedding(q, s, m, group_size=gs, output_dtype=F32).forward(ids)
        got = to_cpu(op.forward(ids.to(DEV)))
        print(f"group_size {gs}: {int((got != want).sum())} of {want.numel()} fp32 values differ")
        assert torch.equal(got, want)
    empty = op.forward(torch.zeros(2, 0, dtype=I64, device=DEV))
    assert empty.shape == (2, 0, 256) and empty.dtype == F32 and empty.is_cuda
