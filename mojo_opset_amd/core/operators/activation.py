"""API class `MojoSwiGLU` (`mojo_opset/core/operators/activation.py:38-66`) and the elementwise `MojoGelu` /
`MojoSilu` (``DIT_BLOCK_OPS``; :6-35)."""
from ..operator import MojoOperator


class MojoSwiGLU(MojoOperator):
    """forward(gate_out, up_out) -> silu(gate_out) * up_out.

    ``swiglu_limit > 0`` first clamps ``up_out`` to ``[-L, L]`` and ``gate_out`` to ``<= L``.
    """

    def __init__(self, swiglu_limit: float = 0.0, **kwargs):
        super().__init__(**kwargs)
        self.swiglu_limit = swiglu_limit

    def extra_repr(self) -> str:
        return f"swiglu_limit={self.swiglu_limit!r}"


class MojoGelu(MojoOperator):
    """forward(x) -> gelu(x) in the erf form (torch's default, not the tanh approximation); any shape, same dtype."""


class MojoSilu(MojoOperator):
    """forward(x) -> x * sigmoid(x); any shape, same dtype."""
