"""mojo_opset_amd — an MI355X-native ``hip`` backend behind the unchanged ``Mojo*`` operator API.

``import mojo_opset_amd`` exposes the `Mojo<Op>` classes of the hot path and
registers the ``HIP<Op>`` backend classes.  Backend selection follows the reference:
``MOJO_BACKEND`` is read at every construction; on a ROCm host the priority is
``["hip", "torch"]``.  The package contains no CPU compute path.

``__all__`` is the SURVEY §8 set, whose torch goldens live in the repo-level ``oracle/`` package.  Ops beyond §8
(``EXTENDED_OPS``: the sliding-window pair ``MojoPagedDecodeSWA`` / ``MojoPagedPrefillSWA``) are package attributes
too, but not in ``__all__``; their goldens are test infrastructure under ``tests/`` (``tests/swa_golden.py``).
So are the ops of the int8 paged KV cache (``KV_INT8_OPS``: ``MojoStorePagedKVCacheC8``,
``MojoPagedDecodeGQAWithKVDequant``, ``MojoPagedPrefillGQAWithKVDequant``; goldens in ``tests/kv_int8_golden.py``).
And sliding-window attention over that cache (``KV_INT8_SWA_OPS``: ``MojoPagedDecodeSWAWithKVDequant``,
``MojoPagedPrefillSWAWithKVDequant``; goldens in ``tests/kv_int8_swa_golden.py``).
And the W8A8 MoE experts (``QUANT_MOE_OPS``: ``MojoMoEDynamicQuant``, ``MojoQuantExperts``, ``MojoQuantMoE``; goldens in
``tests/quant_moe_golden.py``).  And the sampling step (``SAMPLING_OPS``: ``MojoTopKSampling``, ``MojoTopPSampling``,
``MojoTopPFilter``, ``MojoRejectSampling``, ``MojoJoinProbRejectSampling``, ``MojoApplyPenaltiesTempurate``; goldens in
``tests/sampling_golden.py``).  ``plugin.rebase_hip_backend`` registers all six sets into the reference.
"""
from .core import *  # noqa: F401,F403
from .core import __all__ as _core_all
from .core import EXTENDED_OPS, MojoPagedDecodeSWA, MojoPagedPrefillSWA  # noqa: F401
from .core import (KV_INT8_OPS, MojoPagedDecodeGQAWithKVDequant, MojoPagedPrefillGQAWithKVDequant,  # noqa: F401
                   MojoStorePagedKVCacheC8)
from .core import KV_INT8_SWA_OPS, MojoPagedDecodeSWAWithKVDequant, MojoPagedPrefillSWAWithKVDequant  # noqa: F401
from .core import QUANT_MOE_OPS, MojoMoEDynamicQuant, MojoQuantExperts, MojoQuantMoE  # noqa: F401
from .core import (SAMPLING_OPS, MojoApplyPenaltiesTempurate, MojoJoinProbRejectSampling, MojoRejectSampling,  # noqa: F401
                   MojoTopKSampling, MojoTopPFilter, MojoTopPSampling)
from . import backends  # noqa: F401  (registers HIP<Op> classes)
from .paged_cache import PagedDummyCache  # noqa: E402  device-side block allocator

__all__ = list(_core_all) + ["PagedDummyCache"]
__version__ = "0.1.0"
