from .acc import check_tol_diff
from .backend_registry import MojoBackendRegistry
from .operator import MojoOperator
from .operators import *  # noqa: F401,F403
from .operators import __all__ as _ops_all
from .operators import (BEYOND_SURVEY_OPS, EXTENDED_OPS, KV_INT8_OPS, KV_INT8_SWA_OPS, NSTEP_KV_INT8_OPS, NSTEP_OPS,  # noqa: F401
                        DIT_BLOCK_OPS, FULL_ATTN_OPS, PACKED_ATTN_OPS, QUANT_DENSE_OPS, QUANT_MOE_OPS, SAMPLING_OPS, VISION_TOWER_OPS,
                        EMBEDDING_OPS, SHORT_CONV_OPS)
from . import operators as _operators
from .platform import get_dist_backend, get_platform, get_torch_device

__all__ = ["MojoOperator", "MojoBackendRegistry", "check_tol_diff", "get_platform", "get_torch_device",
           "get_dist_backend", *_ops_all]
globals().update({_name: getattr(_operators, _name) for _name in BEYOND_SURVEY_OPS + NSTEP_OPS + NSTEP_KV_INT8_OPS + PACKED_ATTN_OPS + FULL_ATTN_OPS + QUANT_DENSE_OPS + DIT_BLOCK_OPS + VISION_TOWER_OPS + EMBEDDING_OPS + SHORT_CONV_OPS})   # beyond §8: not in __all__
