from .attention import *  # noqa: F401,F403
from .kv_int8 import *  # noqa: F401,F403
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
