from .activation import MojoSwiGLU
from .attention import (MojoPagedDecodeGQA, MojoPagedDecodeGQAWithKVDequant, MojoPagedDecodeSWA,
                        MojoPagedDecodeSWAWithKVDequant, MojoPagedPrefillGQA, MojoPagedPrefillGQAWithKVDequant,
                        MojoPagedPrefillSWA, MojoPagedPrefillSWAWithKVDequant)
from .compute_with_comm import MojoAllGatherGemm, MojoGemmAll2All, MojoGemmAllReduce, MojoGemmReduceScatter
from .gemm import MojoGemm, MojoGroupGemm, MojoQuantGemm
from .kv_cache import (MojoStorePagedKVCache, MojoStorePagedKVCacheC8, MojoStorePagedMLAKVCache,
                       build_paged_kv_chunk_metadata)
from .mla import MojoPagedDecodeMLA, MojoPagedPrefillMLA
from .mlp import MojoSwiGLUMLP
from .moe import MojoExperts, MojoMoE, MojoMoECombine, MojoMoEDispatch, MojoMoEGating, MojoQuantExperts, MojoQuantMoE
from .normalization import MojoResidualAddRMSNorm, MojoRMSNorm, MojoRMSNormInplace
from .position_embedding import MojoApplyRoPE, MojoRotaryEmbedding
from .quantize import MojoDynamicQuant, MojoMoEDynamicQuant, MojoResidualAddRMSNormQuant
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

# Ops beyond the SURVEY §8 set: importable, but not in `__all__` (whose goldens live in the repo-level `oracle/`); their
# goldens are test infrastructure under `tests/`.
EXTENDED_OPS = ("MojoPagedDecodeSWA", "MojoPagedPrefillSWA")
# The int8 paged KV cache with per-channel scales (the reference's experimental "C8" path): same standing as EXTENDED_OPS.
KV_INT8_OPS = ("MojoStorePagedKVCacheC8", "MojoPagedDecodeGQAWithKVDequant", "MojoPagedPrefillGQAWithKVDequant")
# Sliding-window attention over that int8 cache (the product of the two sets above): same standing; goldens in
# tests/kv_int8_swa_golden.py.
KV_INT8_SWA_OPS = ("MojoPagedDecodeSWAWithKVDequant", "MojoPagedPrefillSWAWithKVDequant")
# W8A8 MoE experts (the reference's quantised MoE: per-expert smooth quantiser, int8 experts, the layer): same standing again;
# goldens in tests/quant_moe_golden.py.
QUANT_MOE_OPS = ("MojoMoEDynamicQuant", "MojoQuantExperts", "MojoQuantMoE")
# The sampling step (top-k / top-p over the vocabulary, speculative acceptance, penalties): same standing once more; goldens
# in tests/sampling_golden.py.
SAMPLING_OPS = ("MojoTopKSampling", "MojoTopPSampling", "MojoTopPFilter", "MojoRejectSampling", "MojoJoinProbRejectSampling",
                "MojoApplyPenaltiesTempurate")
