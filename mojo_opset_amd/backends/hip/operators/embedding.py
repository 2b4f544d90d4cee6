"""HIP<Op> classes of the input-embedding ops (`EMBEDDING_OPS`): the plain and the vocabulary-parallel embedding, the packed-NF4
lookup, the n-gram ids of the over-encoding layer and the layer itself (csrc/embedding.hip).  Each `forward`
validates the contract before any device call, hands raw device pointers to the C ABI and returns torch tensors.  Ids, ``q_lens``
and the layer's vocabulary buffers are read on the device: no forward synchronises with the host."""
from typing import Optional

import torch
import torch.distributed as dist

from ....core.operators.embedding import MojoEmbedding, MojoParallelEmbedding, is_dist_initialized
from ....core.operators.over_encoding import (MojoNF4DequantEmbedding, MojoOverEncoding, MojoOverEncodingNGram,
                                              check_oe_call_contract)
from .. import lib as L
from .gemm import dense_gemm

_ROCM = ["rocm"]
_FLOATS = (torch.float32, torch.bfloat16, torch.float16)
_INDEX = (torch.int32, torch.int64)


def _index_tensor(what: str, name: str, t: torch.Tensor, dense: bool = True) -> torch.Tensor:
    if t.dtype not in _INDEX:
        raise NotImplementedError(f"{what}: {name} must be int32 or int64, got {t.dtype}")
    return t.contiguous() if dense else t


def _rows(t: torch.Tensor):
    """``(tensor, row stride in elements)`` of a 2-D tensor the kernels read in place: the last dimension dense and the rows apart
    by at least a row (a column slice of a wider tensor qualifies).  Anything else — a transposed view, an expanded or overlapping
    one (``row.expand(B, H)`` has strides (0, 1)) — is copied.  The stride of a one-row tensor is arbitrary and never used."""
    rows, cols = t.shape
    if (cols > 1 and t.stride(1) != 1) or (rows > 1 and t.stride(0) < cols):
        t = t.contiguous()
    return t, (t.stride(0) if rows > 1 else cols)


def _is_i64(t: torch.Tensor) -> int:
    return 1 if t.dtype == torch.int64 else 0


def _gather(what: str, ids: torch.Tensor, table: torch.Tensor, vocab_start: int) -> torch.Tensor:
    """``table[ids - vocab_start]``, zeros outside the table: `mojo_hip_embedding`.  The table is read in place through its row
    stride (a column slice of a wider table qualifies)."""
    if table.dim() != 2:
        raise ValueError(f"{what}: the table must be 2-D, got {tuple(table.shape)}")
    if table.dtype not in _FLOATS:
        raise NotImplementedError(f"{what}: table dtype {table.dtype}; float32, bfloat16 and float16 are supported")
    ids = _index_tensor(what, "input", ids)
    L.require_cuda(ids, table)
    table, table_stride = _rows(table)
    rows, dim = table.shape
    out = torch.empty(*ids.shape, dim, dtype=table.dtype, device=table.device)
    if out.numel():
        L.check(L.load().mojo_hip_embedding(L.ptr(ids), _is_i64(ids), L.ptr(table), L.ptr(out), ids.numel(), rows, dim,
                                            int(vocab_start), table_stride, dim, L.dtype_code(table.dtype),
                                            L.stream_of(table)), what)
    return out


class HIPEmbedding(MojoEmbedding):
    """One launch copies ``weight[input]`` (16-byte vectors when the row allows it).  ``padding_idx`` has no effect in a forward
    pass.  Deviation: an index outside ``[0, num_embeddings)`` gives a row of ZEROS where the reference raises (a device-side
    assert is not acceptable on a shared GPU, and a host check would synchronise).  ``max_norm`` rewrites the table in place in
    torch: `NotImplementedError`."""
    supported_platforms_list = _ROCM

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        if self.max_norm is not None:
            raise NotImplementedError("HIPEmbedding: max_norm (an in-place renormalisation of the table) is not implemented")
        return _gather("HIPEmbedding", input, self.weight.detach(), 0)


class HIPParallelEmbedding(MojoParallelEmbedding):
    """The local shard's rows, zeros for an index another rank owns (the reference's semantics, in the same launch as the
    lookup), then the reference's ``all_reduce`` when a process group is initialised."""
    supported_platforms_list = _ROCM

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        if self.max_norm is not None:
            raise NotImplementedError("HIPParallelEmbedding: max_norm is not implemented")
        out = _gather("HIPParallelEmbedding", input, self.weight.detach(), self.vocab_start_index)
        if is_dist_initialized():
            dist.all_reduce(out, op=dist.ReduceOp.SUM, group=self.process_group)
        return out


def _nf4_tables(what: str, op):
    """``(qweight, scale, mean, codebook fp16)`` of an NF4 module, dense, validated."""
    q, scale, mean = op.weight.detach(), op.scale.detach(), op.mean.detach()
    if q.dtype not in (torch.int8, torch.uint8):
        raise ValueError(f"{what}: the packed table must be int8 or uint8, got {q.dtype}")
    if scale.dtype not in _FLOATS or mean.dtype != scale.dtype:
        raise NotImplementedError(f"{what}: scale and mean must share one of float32 / bfloat16 / float16, got {scale.dtype} "
                                  f"and {mean.dtype}")
    codebook = op.codebook.detach()
    if tuple(codebook.shape) != (16,):
        raise ValueError(f"{what}: the codebook must hold 16 levels, got {tuple(codebook.shape)}")
    return q.contiguous(), scale.contiguous(), mean.contiguous(), codebook.to(torch.float16).contiguous()


class HIPNF4DequantEmbedding(MojoNF4DequantEmbedding):
    """One launch gathers and dequantises: ``fp32(codebook[nibble]) * fp32(scale) + fp32(mean)`` with the module's fp16
    codebook, the product and the sum rounded separately, one rounding to ``output_dtype`` — the reference's bits.  Zeros for an
    id outside ``[vocab_start_id, vocab_start_id + rows)``.  ``cpu_only=True``: `NotImplementedError` (no CPU compute path)."""
    supported_platforms_list = _ROCM

    def __init__(self, qweight, scale, mean, *, group_size, vocab_start_id=0, cpu_only=False,
                 output_dtype=torch.bfloat16, **kwargs):
        if cpu_only:
            raise NotImplementedError("HIPNF4DequantEmbedding: cpu_only=True (a CPU-resident table) is not implemented")
        super().__init__(qweight, scale, mean, group_size=group_size, vocab_start_id=vocab_start_id, cpu_only=cpu_only,
                         output_dtype=output_dtype, **kwargs)

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        what = "HIPNF4DequantEmbedding"
        if self.output_dtype not in _FLOATS:
            raise NotImplementedError(f"{what}: output_dtype {self.output_dtype}; float32, bfloat16 and float16 are supported")
        q, scale, mean, codebook = _nf4_tables(what, self)
        ids = _index_tensor(what, "input", input)
        if ids.numel() == 0:
            return torch.empty((*input.shape, self.embedding_dim), dtype=self.output_dtype, device=input.device)
        L.require_cuda(ids, q, scale, mean, codebook)
        dim = self.embedding_dim
        out = torch.empty(*ids.shape, dim, dtype=self.output_dtype, device=q.device)
        L.check(L.load().mojo_hip_nf4_embedding(L.ptr(ids), _is_i64(ids), L.ptr(q), L.ptr(scale), L.ptr(mean), L.ptr(codebook),
                                                L.ptr(out), ids.numel(), q.shape[0], dim, int(self.group_size),
                                                int(self.vocab_start_id), dim, L.dtype_code(scale.dtype),
                                                L.dtype_code(self.output_dtype), L.stream_of(q)), what)
        return out


def _max_gram(op) -> int:
    """The largest gram, a host quantity: read from the ``oe_grams`` buffer (one synchronisation) and kept for as long as that
    buffer is the same tensor with the same contents — torch counts every in-place write (a `load_state_dict` copies in place)
    in ``_version``, and an assignment or a move gives another tensor — so a forward after the first makes no synchronisation
    and a changed buffer is read again."""
    grams = op.oe_grams
    key = (grams.data_ptr(), grams._version, grams.numel())
    cached = op.__dict__.get("_hip_max_gram")
    if cached is None or cached[0] != key:
        cached = (key, max([int(g) for g in grams.tolist()] + [1]))
        op.__dict__["_hip_max_gram"] = cached
    return cached[1]


def _ngram_call(what: str, op, input_ids, history, q_lens):
    """Validation shared by the id launch and the fused one; returns the leading arguments of both C entry points."""
    check_oe_call_contract(input_ids, history, q_lens, _max_gram(op))
    sizes, grams, offsets = op.oe_vocab_sizes, op.oe_grams, op.oe_vocab_offsets
    for name, t in (("oe_vocab_sizes", sizes), ("oe_grams", grams), ("oe_vocab_offsets", offsets)):
        if t.dtype not in _INDEX:
            raise NotImplementedError(f"{what}: {name} must be int32 or int64, got {t.dtype}")
    if not (sizes.numel() == grams.numel() == offsets.numel()) or sizes.numel() == 0:
        raise ValueError(f"{what}: oe_vocab_sizes, oe_grams and oe_vocab_offsets must hold one entry per vocabulary")
    ids = _index_tensor(what, "input_ids", input_ids)
    hist, hist_stride = _rows(_index_tensor(what, "oe_history_input", history, dense=False))
    lens = None if q_lens is None else _index_tensor(what, "q_lens", q_lens)
    L.require_cuda(ids, hist, lens, sizes, grams, offsets)
    sizes, grams, offsets = sizes.contiguous(), grams.contiguous(), offsets.contiguous()
    batch = hist.shape[0]
    seq_len = 0 if lens is not None else ids.shape[1]
    flags = (_is_i64(ids) | _is_i64(hist) << 1 | (_is_i64(lens) << 2 if lens is not None else 0) | _is_i64(sizes) << 3 |
             _is_i64(grams) << 4 | _is_i64(offsets) << 5)
    keep = (ids, hist, lens, sizes, grams, offsets)
    lead = (L.ptr(ids), L.ptr(hist), L.ptr(lens), L.ptr(sizes), L.ptr(grams), L.ptr(offsets))
    tail = (ids.numel(), batch, seq_len, hist.shape[1], hist_stride,
            sizes.numel(), _max_gram(op), int(op.ori_vocab_size), flags)
    return keep, lead, tail


class HIPOverEncodingNGram(MojoOverEncodingNGram):
    """One launch, one thread per (token, vocabulary); a packed token's sequence is found on the device from ``q_lens`` (the
    reference loops over the sequences on the host with an ``.item()`` each).  64-bit arithmetic; the output has the dtype of
    ``input_ids``.  A history shorter than ``max gram - 1``: `ValueError`."""
    supported_platforms_list = _ROCM

    def forward(self, input_ids: torch.Tensor, oe_history_input: torch.Tensor, q_lens: Optional[torch.Tensor] = None):
        keep, lead, tail = _ngram_call("HIPOverEncodingNGram", self, input_ids, oe_history_input, q_lens)
        ids = keep[0]
        out = torch.empty(*ids.shape, tail[5], dtype=ids.dtype, device=ids.device)
        if out.numel():
            L.check(L.load().mojo_hip_oe_ngram(*lead, L.ptr(out), *tail, L.stream_of(ids)), "HIPOverEncodingNGram")
        return out


def over_encoding_concat(layer, input_tensor: torch.Tensor, oe_history_input: torch.Tensor,
                         q_lens: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The operand of the up projection, ``[..., ori_embed_dim + G * oe_embed_dim]``, in ONE launch
    (`mojo_hip_over_encoding_concat`): per token the original table's row and the mega table's rows of its ``G`` n-gram ids,
    which are computed in the same launch and never written.  ``layer`` is a `MojoOverEncoding` (dense or NF4 mega table).
    Bit for bit the concatenation of the separate launches `HIPOverEncodingNGram` -> `HIPEmbedding` / `HIPNF4DequantEmbedding`."""
    what = "HIPOverEncoding"
    if getattr(layer, "mega_embedding_cpu_only", False):
        raise NotImplementedError(f"{what}: mega_embedding_cpu_only=True (a CPU-resident mega table) is not implemented")
    ori = layer.ori_embedding.weight.detach()
    mega = layer.oe_mega_embedding
    nf4 = isinstance(mega, MojoNF4DequantEmbedding) or hasattr(mega, "codebook")
    dtype = ori.dtype
    if dtype not in _FLOATS:
        raise NotImplementedError(f"{what}: table dtype {dtype}; float32, bfloat16 and float16 are supported")
    if ori.dim() != 2:
        raise ValueError(f"{what}: the original table must be 2-D")
    if nf4:
        table, scale, mean, codebook = _nf4_tables(what, mega)
        if mega.output_dtype is not None and mega.output_dtype != dtype:
            raise NotImplementedError(f"{what}: the NF4 mega table dequantises to {mega.output_dtype}, the original table is "
                                      f"{dtype}: tables and projection must share one dtype")
        mega_dim, group, start, sm_code = int(mega.embedding_dim), int(mega.group_size), int(mega.vocab_start_id), L.dtype_code(scale.dtype)
        mega_stride = mega_dim
    else:
        table, scale, mean, codebook = mega.weight.detach(), None, None, None
        if table.dtype != dtype:
            raise NotImplementedError(f"{what}: the mega table is {table.dtype}, the original table {dtype}: tables and projection "
                                      f"must share one dtype")
        table, mega_stride = _rows(table)
        mega_dim, group, start, sm_code = table.shape[1], 1, 0, 0
    ori, ori_stride = _rows(ori)
    keep, lead, tail = _ngram_call(what, layer, input_tensor, oe_history_input, q_lens)
    L.require_cuda(ori, table, scale, mean, codebook)
    ids = keep[0]
    width = ori.shape[1] + tail[5] * mega_dim
    out = torch.empty(*ids.shape, width, dtype=dtype, device=ori.device)
    if out.numel():
        L.check(L.load().mojo_hip_over_encoding_concat(
            *lead, *tail, L.ptr(ori), ori.shape[0], ori.shape[1], ori_stride, L.ptr(table), L.ptr(scale),
            L.ptr(mean), L.ptr(codebook), table.shape[0], mega_dim, mega_stride, group, start, 1 if nf4 else 0, sm_code,
            L.ptr(out), width, L.dtype_code(dtype), L.stream_of(ori)), what)
    return out


class HIPOverEncoding(MojoOverEncoding):
    """Two launches: `over_encoding_concat` (ids, the original row and the ``G`` mega rows of every token, written straight into
    the concatenation) and the dense GEMM with ``oe_up_proj``.  The reference composes about 60 torch launches and, with
    ``q_lens``, loops over the sequences on the host.  Dense or NF4 mega table; tables and projection share one of float32 /
    bfloat16 / float16; ``mega_embedding_cpu_only=True``: `NotImplementedError`."""
    supported_platforms_list = _ROCM

    def _nf4_embedding_class(self):
        return HIPNF4DequantEmbedding

    def forward(self, input_tensor: torch.Tensor, oe_history_input: torch.Tensor, q_lens: Optional[torch.Tensor] = None):
        weight = self.oe_up_proj.weight.detach()
        if weight.dtype != self.ori_embedding.weight.dtype:
            raise NotImplementedError(f"HIPOverEncoding: oe_up_proj is {weight.dtype}, the original table "
                                      f"{self.ori_embedding.weight.dtype}: tables and projection must share one dtype")
        concat = over_encoding_concat(self, input_tensor, oe_history_input, q_lens)
        return dense_gemm(concat, weight, None, trans_weight=False)
