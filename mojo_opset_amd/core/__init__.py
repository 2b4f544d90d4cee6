from .acc import check_tol_diff
from .backend_registry import MojoBackendRegistry
from .operator import MojoOperator
from .operators import *  # noqa: F401,F403
from .operators import __all__ as _ops_all
from .operators import EXTENDED_OPS, MojoPagedDecodeSWA, MojoPagedPrefillSWA  # noqa: F401  (beyond §8: not in __all__)
from .operators import (KV_INT8_OPS, MojoPagedDecodeGQAWithKVDequant, MojoPagedPrefillGQAWithKVDequant,  # noqa: F401
                        MojoStorePagedKVCacheC8)
from .operators import KV_INT8_SWA_OPS, MojoPagedDecodeSWAWithKVDequant, MojoPagedPrefillSWAWithKVDequant  # noqa: F401
from .operators import QUANT_MOE_OPS, MojoMoEDynamicQuant, MojoQuantExperts, MojoQuantMoE  # noqa: F401
from .operators import (SAMPLING_OPS, MojoApplyPenaltiesTempurate, MojoJoinProbRejectSampling, MojoRejectSampling,  # noqa: F401
                        MojoTopKSampling, MojoTopPFilter, MojoTopPSampling)
from .platform import get_dist_backend, get_platform, get_torch_device

__all__ = ["MojoOperator", "MojoBackendRegistry", "check_tol_diff", "get_platform", "get_torch_device",
           "get_dist_backend", *_ops_all]
