from .attention import *  # noqa: F401,F403
from .kv_int8 import *  # noqa: F401,F403
from .sage import HIPPagedPrefillSageGQA  # noqa: F401
from .nsa import HIPDecodeNSA, HIPPagedDecodeNSA, HIPPagedPrefillNSA, HIPPrefillNSA  # noqa: F401
from .linear_attention import HIPGatedDeltaRule, HIPGatedDeltaRuleUpdateState  # noqa: F401
from .mxfp4 import HIPMXFP4Experts, HIPMXFP4Gemm, HIPMXFP4GroupGemm, HIPMXFP4Quant, HIPMXFP4SwiGLUQuant  # noqa: F401
from .convolution import HIPCausalConv1d, HIPCausalConv1dUpdateState  # noqa: F401
from .embedding import (HIPEmbedding, HIPNF4DequantEmbedding, HIPOverEncoding, HIPOverEncodingNGram,  # noqa: F401
                        HIPParallelEmbedding)
from .gemm import HIPGemm, HIPGroupGemm, HIPQuantGemm, HIPSwiGLUMLP  # noqa: F401
from .streaming import *  # noqa: F401,F403
from .mla import *  # noqa: F401,F403
from .compute_with_comm import *  # noqa: F401,F403
from .moe import *  # noqa: F401,F403
from .quantize import *  # noqa: F401,F403
from .sampling import (HIPApplyPenaltiesTempurate, HIPJoinProbRejectSampling, HIPRejectSampling, HIPTopKSampling,  # noqa: F401
                       HIPTopPFilter, HIPTopPSampling)
