"""mojo_opset_amd — an MI355X-native ``hip`` backend behind the unchanged ``Mojo*`` operator API.

``import mojo_opset_amd`` exposes the `Mojo<Op>` classes of the hot path and
registers the ``HIP<Op>`` backend classes.  Backend selection follows the reference:
``MOJO_BACKEND`` is read at every construction; on a ROCm host the priority is
``["hip", "torch"]``.  The package contains no CPU compute path.

``__all__`` is the SURVEY §8 set.  The ops beyond it (``BEYOND_SURVEY_OPS``, the concatenation of the named sets of
``core/operators/__init__.py``) are package attributes too, but not in ``__all__``; ``plugin.rebase_hip_backend``
registers both into the reference.  The torch golden of every op, in ``__all__`` or not, is in the repo-level ``oracle/``
package.  ``NSTEP_OPS`` (n-step paged decode) is a further set of package attributes the plugin registers; its torch golden
is ``tests/nstep_golden.py``.  ``NSTEP_KV_INT8_OPS`` (the same over the int8 cache) is one more such set; its golden is
``tests/nstep_kv_int8_golden.py``.  ``PACKED_ATTN_OPS`` (`MojoSWA`: packed var-len attention over contiguous K/V) is another;
its golden is ``tests/swa_packed_golden.py``.  ``FULL_ATTN_OPS`` (`MojoSdpa`: bidirectional attention with an optional mask) is
another; its golden is ``tests/sdpa_golden.py``.  ``QUANT_DENSE_OPS`` (the activation ops between the GEMMs of a dense W8A8 layer:
norm + quant, static quant, dequant, dequant -> SwiGLU -> quant) is one more; its golden is ``tests/quant_dense_golden.py``.
``DIT_BLOCK_OPS`` (the ops around every attention of a DiT block: LayerNorm, residual-add LayerNorm, GELU, SiLU, grid RoPE) is
one more; its golden is ``tests/dit_block_golden.py``.  ``VISION_TOWER_OPS`` (what a Qwen-VL model adds: packed var-len bidirectional
attention, the vision tower's 2-D rotary pair, the decoder's multimodal RoPE) is one more; its golden is
``tests/vision_tower_golden.py``.  ``EMBEDDING_OPS`` (token ids to hidden states: the plain and the vocabulary-parallel
embedding, the over-encoding layer with its n-gram ids and the packed-NF4 lookup) is one more; its golden is
``tests/embedding_golden.py``.  ``SHORT_CONV_OPS`` (the depthwise causal short convolution in front of a linear-attention or
state-space mixer: the prefill forward and the state update) is one more; its golden is ``tests/short_conv_golden.py``.
"""
from .core import *  # noqa: F401,F403
from .core import __all__ as _core_all
from .core import (BEYOND_SURVEY_OPS, EXTENDED_OPS, KV_INT8_OPS, KV_INT8_SWA_OPS, NSTEP_KV_INT8_OPS, NSTEP_OPS,  # noqa: F401
                   DIT_BLOCK_OPS, FULL_ATTN_OPS, PACKED_ATTN_OPS, QUANT_DENSE_OPS, QUANT_MOE_OPS, SAMPLING_OPS, VISION_TOWER_OPS,
                   EMBEDDING_OPS, SHORT_CONV_OPS)
from . import core as _core
from . import backends  # noqa: F401  (registers HIP<Op> classes)
from .paged_cache import PagedDummyCache  # noqa: E402  device-side block allocator

__all__ = list(_core_all) + ["PagedDummyCache"]
globals().update({_name: getattr(_core, _name) for _name in BEYOND_SURVEY_OPS + NSTEP_OPS + NSTEP_KV_INT8_OPS + PACKED_ATTN_OPS + FULL_ATTN_OPS + QUANT_DENSE_OPS + DIT_BLOCK_OPS + VISION_TOWER_OPS + EMBEDDING_OPS + SHORT_CONV_OPS})   # beyond §8: not in __all__
__version__ = "0.1.0"
