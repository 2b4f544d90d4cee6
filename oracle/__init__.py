"""ORACLE — TEST INFRASTRUCTURE, NOT PRODUCT.

CPU restatement (plain PyTorch, fp32 softmax / reference rounding points) of the reference's
torch-native golden backend for every op of the package: the hot path in
``torch_golden``, the ops beyond it (`mojo_opset_amd.core.operators.BEYOND_SURVEY_OPS`) in ``swa``,
``kv_int8``, ``kv_int8_swa``, ``quant_moe`` and ``sampling``, their shared paged-cache helpers in
``paged``.  Importing this package registers a ``Torch<Op>`` class — backend name ``"torch"`` — into
the registry of each `mojo_opset_amd.core.Mojo<Op>`, whatever was imported before, which is how the
parity tests obtain ``Mojo<Op>._registry.get("torch")`` exactly as the reference's tests do.
``__all__`` is the §8 class list; the other modules are reached by name (``oracle.swa``, ...).

Only ``tests/``, ``benchmarks/``, ``__graft_entry__.smoke()`` and ``bench.py``'s ``cpu_baseline``
leg may import it.  Nothing under ``mojo_opset_amd/`` imports it: the product path never computes
on the CPU.

Parity pin: every function here is checked bit-for-bit (`torch.equal`) against outputs captured
from the imported reference (`/root/reference`, torch 2.10.0+rocm7.0 CPU) — see
``oracle/make_golden.py`` and ``oracle/make_*_golden.py`` (the generators, run in the authoring
container) and ``tests/golden/*.pt`` (the captured vectors) — plus the reference's own known-answer tests
re-stated in ``tests/test_oracle_kat.py``.  One exception: fp8 `MojoQuantGemm` has no reference
implementation — **parity unpinned** for that dtype (its restatement is checked against an
independent float64 formula only).
"""
from . import kv_int8, kv_int8_swa, paged, quant_moe, sampling, swa  # noqa: F401
from .torch_golden import *  # noqa: F401,F403
from .torch_golden import __all__  # noqa: F401
