from .activation import MojoGelu, MojoSilu, MojoSwiGLU
from .attention import (MojoPagedDecodeGQA, MojoPagedDecodeGQAWithKVDequant, MojoPagedDecodeNstepSWA,
                        MojoPagedDecodeNstepSWAWithKVDequant, MojoPagedDecodeSWA, MojoPagedDecodeSWAWithKVDequant,
                        MojoPagedPrefillGQA, MojoPagedPrefillGQAWithKVDequant,
                        MojoPagedPrefillSWA, MojoPagedPrefillSWAWithKVDequant, MojoPackedSdpa, MojoSdpa,
                        MojoSWA)
from .compute_with_comm import MojoAllGatherGemm, MojoGemmAll2All, MojoGemmAllReduce, MojoGemmReduceScatter
from .convolution import MojoCausalConv1d, MojoCausalConv1dUpdateState
from .embedding import MojoEmbedding, MojoParallelEmbedding
from .gemm import MojoGemm, MojoGroupGemm, MojoQuantGemm
from .kv_cache import (MojoStorePagedKVCache, MojoStorePagedKVCacheC8, MojoStorePagedMLAKVCache,
                       build_paged_kv_chunk_metadata)
from .mla import MojoPagedDecodeMLA, MojoPagedPrefillMLA
from .mlp import MojoSwiGLUMLP
from .moe import MojoExperts, MojoMoE, MojoMoECombine, MojoMoEDispatch, MojoMoEGating, MojoQuantExperts, MojoQuantMoE
from .over_encoding import MojoNF4DequantEmbedding, MojoOverEncoding, MojoOverEncodingNGram
from .normalization import (MojoLayerNorm, MojoResidualAddLayerNorm, MojoResidualAddRMSNorm, MojoRMSNorm,
                            MojoRMSNormInplace)
from .position_embedding import (MojoApplyRoPE, MojoApplyVisionRoPE2D, MojoGridRoPE, MojoMRoPE, MojoMRoPEInplace,
                                 MojoRotaryEmbedding, MojoVisionRotaryEmbedding2D)
from .quantize import (MojoDequant, MojoDequantSwiGLUQuant, MojoDynamicQuant, MojoLayerNormQuant, MojoMoEDynamicQuant,
                       MojoResidualAddLayerNormQuant, MojoResidualAddRMSNormQuant, MojoRMSNormQuant, MojoStaticQuant)
from .sampling import (MojoApplyPenaltiesTempurate, MojoJoinProbRejectSampling, MojoRejectSampling, MojoTopKSampling,
                       MojoTopPFilter, MojoTopPSampling)

__all__ = [
    "MojoSwiGLU", "MojoPagedDecodeGQA", "MojoPagedPrefillGQA", "MojoAllGatherGemm", "MojoGemmAll2All",
    "MojoGemmAllReduce", "MojoGemmReduceScatter", "MojoGroupGemm", "MojoQuantGemm", "MojoStorePagedKVCache",
    "build_paged_kv_chunk_metadata", "MojoPagedDecodeMLA", "MojoPagedPrefillMLA", "MojoResidualAddRMSNorm",
    "MojoRMSNorm", "MojoRMSNormInplace", "MojoApplyRoPE", "MojoRotaryEmbedding", "MojoMoEGating", "MojoMoEDispatch", "MojoExperts",
    "MojoMoECombine", "MojoMoE", "MojoDynamicQuant", "MojoResidualAddRMSNormQuant", "MojoStorePagedMLAKVCache",
    "MojoGemm", "MojoSwiGLUMLP",
]

# Ops beyond the SURVEY §8 set: attributes of the package, but not in `__all__`.  Their torch goldens are in `oracle/`, like
# those of `__all__`.  A new set gets a tuple of its own here and joins BEYOND_SURVEY_OPS, which is what the packages above
# re-export and what the plugin registers.
EXTENDED_OPS = ("MojoPagedDecodeSWA", "MojoPagedPrefillSWA")                        # sliding-window attention
# the int8 paged KV cache with per-channel scales (the reference's experimental "C8" path)
KV_INT8_OPS = ("MojoStorePagedKVCacheC8", "MojoPagedDecodeGQAWithKVDequant", "MojoPagedPrefillGQAWithKVDequant")
KV_INT8_SWA_OPS = ("MojoPagedDecodeSWAWithKVDequant", "MojoPagedPrefillSWAWithKVDequant")   # the product of the two above
# W8A8 MoE experts: per-expert smooth quantiser, int8 experts, the layer
QUANT_MOE_OPS = ("MojoMoEDynamicQuant", "MojoQuantExperts", "MojoQuantMoE")
# the sampling step: top-k / top-p over the vocabulary, speculative acceptance, penalties
SAMPLING_OPS = ("MojoTopKSampling", "MojoTopPSampling", "MojoTopPFilter", "MojoRejectSampling", "MojoJoinProbRejectSampling",
                "MojoApplyPenaltiesTempurate")
BEYOND_SURVEY_OPS = EXTENDED_OPS + KV_INT8_OPS + KV_INT8_SWA_OPS + QUANT_MOE_OPS + SAMPLING_OPS
# multi-token (n-step) paged decode: scores the draft run the sampling ops accept or reject.  A package attribute and a
# plugin-registered class like the sets above, but not part of BEYOND_SURVEY_OPS: its torch golden is tests/nstep_golden.py,
# not yet a module of `oracle/`.
NSTEP_OPS = ("MojoPagedDecodeNstepSWA",)
# the n-step decode over the int8 cache: a set of its own for the same reason (golden: tests/nstep_kv_int8_golden.py)
NSTEP_KV_INT8_OPS = ("MojoPagedDecodeNstepSWAWithKVDequant",)
# packed var-len attention over contiguous K/V (the reference's core `MojoSWA`): a set of its own likewise (golden:
# tests/swa_packed_golden.py)
PACKED_ATTN_OPS = ("MojoSWA",)
# bidirectional attention with an optional mask (the reference's core `MojoSdpa`): a set of its own likewise (golden:
# tests/sdpa_golden.py)
FULL_ATTN_OPS = ("MojoSdpa",)
# the activation ops between the GEMMs of a dense W8A8 decoder layer: norm + quant, static quant, dequant and the fc1 -> fc2
# stage.  A set of its own likewise (golden: tests/quant_dense_golden.py)
QUANT_DENSE_OPS = ("MojoRMSNormQuant", "MojoLayerNormQuant", "MojoResidualAddLayerNormQuant", "MojoStaticQuant", "MojoDequant",
                   "MojoDequantSwiGLUQuant")
# the ops around every `MojoSdpa` of a DiT block (Wan2.2): LayerNorm with and without affine, the FFN's GELU, the time
# embedding's SiLU and the 3-D grid RoPE of q and k.  A set of its own likewise (golden: tests/dit_block_golden.py)
DIT_BLOCK_OPS = ("MojoLayerNorm", "MojoResidualAddLayerNorm", "MojoGelu", "MojoSilu", "MojoGridRoPE")
# the ops a Qwen-VL model adds to the text decoder: packed var-len bidirectional attention (the vision tower's, with the
# semantics of the reference's `MojoSWA(is_causal=False)`), the tower's 2-D rotary pair and the decoder's multimodal RoPE.  A set
# of its own likewise (golden: tests/vision_tower_golden.py)
VISION_TOWER_OPS = ("MojoPackedSdpa", "MojoVisionRotaryEmbedding2D", "MojoApplyVisionRoPE2D", "MojoMRoPE", "MojoMRoPEInplace")
# the first operation of a decode step: token ids to hidden states.  The plain and the vocabulary-parallel embedding lookup, the
# over-encoding layer (n-gram ids, the fused gather of the original and the mega table's rows, the up projection) and the
# packed-NF4 lookup its mega table may be stored as.  A set of its own likewise (golden: tests/embedding_golden.py)
EMBEDDING_OPS = ("MojoEmbedding", "MojoParallelEmbedding", "MojoOverEncodingNGram", "MojoOverEncoding", "MojoNF4DequantEmbedding")
# the depthwise causal "short convolution" (width 2..4, optional SiLU) in front of every linear-attention or state-space mixer:
# the reference's update-state op and the forward of its `MojoCausalConv1dFunction` as an inference operator (the reference has no
# operator class of that name).  A set of its own likewise (golden: tests/short_conv_golden.py)
SHORT_CONV_OPS = ("MojoCausalConv1dUpdateState", "MojoCausalConv1d")
