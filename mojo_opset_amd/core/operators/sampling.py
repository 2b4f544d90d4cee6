"""API classes of the sampling step: from a row of logits to a token (beyond the SURVEY §8 set: `SAMPLING_OPS`).

Follows `mojo_opset/core/operators/sampling.py`: `MojoTopKSampling` (:12-71), `MojoTopPSampling` (:74-144), `MojoTopPFilter`
(:147-206), `MojoRejectSampling` (:209-253), `MojoJoinProbRejectSampling` (:256-307), `MojoApplyPenaltiesTempurate`
(:310-361).  Constructors, call contracts and ``extra_repr`` only; the torch goldens are `oracle/sampling.py`, the
kernels `csrc/sampling.hip`.

Shared semantics (all in fp32 on ``logits.float()``):

* top-k stage: the ``K`` largest values of the last dimension in descending order with their int64 indices; among equal
  values the LOWER index comes first, and a tie that straddles position ``K`` keeps the lower indices;
* nucleus mask over those ``K``: ``remove = cumsum(softmax(values)) > top_p``; the first ``min_tokens_to_keep - 1`` positions
  are cleared when ``min_tokens_to_keep > 1``; the mask moves one position right and position 0 is never removed; removed
  positions take ``filter_value`` (finite values keep a share of the second softmax); ``final_probs_dist`` is the softmax of
  the result.
"""
from ..operator import MojoOperator


class MojoTopKSampling(MojoOperator):
    """forward(logits [..., V]) -> (next_probs fp32 [..., 1], next_tokens int64 [..., 1]): one draw per row from the softmax
    of the top ``K = max(min(top_k, V), min_tokens_to_keep)`` logits.  ``filter_value`` is stored and unused, as in the
    reference."""

    def __init__(self, top_k: int = 50, filter_value: float = -float("Inf"), min_tokens_to_keep: int = 1,
                 op_name: str = "", layer_idx: int = 0):
        super().__init__()
        self.op_name = op_name
        self.layer_idx = layer_idx
        self.top_k = top_k
        self.filter_value = filter_value
        self.min_tokens_to_keep = min_tokens_to_keep

    def effective_k(self, vocab: int) -> int:
        return max(min(self.top_k, vocab), self.min_tokens_to_keep)


class MojoTopPSampling(MojoOperator):
    """forward(logits [..., V]) -> (next_probs fp32 [..., 1], next_tokens int64 [..., 1]): one draw per row from
    ``final_probs_dist`` of the nucleus mask over the top ``K = min(rand_top_k, V)`` logits."""

    def __init__(self, top_p: float = 0.75, filter_value: float = -float("Inf"), min_tokens_to_keep: int = 1,
                 rand_top_k: int = 1000):
        super().__init__()
        self.top_p = top_p
        self.filter_value = filter_value
        self.min_tokens_to_keep = min_tokens_to_keep
        self.rand_top_k = rand_top_k

    def extra_repr(self) -> str:
        return (f"top_p={self.top_p}, filter_value={self.filter_value}, min_tokens_to_keep={self.min_tokens_to_keep}, "
                f"rand_top_k={self.rand_top_k}")


class MojoTopPFilter(MojoOperator):
    """forward(logits [..., V], top_p, min_tokens_to_keep, rand_top_k) -> (final_probs_dist [..., K] in the input dtype,
    indices int64 [..., K]) with ``K = min(rand_top_k, V)``: the nucleus mask without the draw."""

    def __init__(self, filter_value: float = -float("Inf")):
        super().__init__()
        self.filter_value = filter_value

    def extra_repr(self) -> str:
        return f"filter_value={self.filter_value}"


class MojoRejectSampling(MojoOperator):
    """forward(target_probs [B, S+1, V], draft_tokens int64 [B, S], draft_probs [B, S], random_seed=None)
    -> (next_tokens int64 [B, S+1] = [draft_tokens | 0], accepted_len int64 [B]).

    ONE uniform ``u`` per row; draft token ``j`` is rejected when ``target_probs[b, j, draft_tokens[b, j]] / draft_probs[b, j]
    < u``; ``accepted_len`` is the index of the first rejected token, ``S`` when none is."""


class MojoJoinProbRejectSampling(MojoOperator):
    """forward(target_probs [B, S+1, V], draft_tokens int64 [B, S], draft_probs [B, S], random_seed=None)
    -> (next_tokens int64 [B, S+1] = [draft_tokens | 0], accepted_len int32 [B]).

    ``S`` uniforms per row; with ``pi = cumprod(clamp(target / draft, 0, 1))`` and ``r = cumprod(uniforms)`` along the row,
    position ``j`` is rejected when ``pi[j] < r[j]``; ``accepted_len`` is one past the LAST position that is not rejected
    (0 when every one is) — not the length of the accepted prefix: a later acceptance overrides an earlier rejection."""


class MojoApplyPenaltiesTempurate(MojoOperator):
    """forward(logits [B, V], token_freqs, presence_penalties, frequency_penalties, repetition_penalties, temps=None).

    Per row ``i``, in fp32 and in this order; the first three only where ``token_freqs[i]`` (``[V]``) is not ``None``:
    ``l -= frequency_penalties[i] * freq`` (unless the penalty is 0), ``l -= presence_penalties[i] * (freq > 0)`` (unless 0),
    then by the sign of ``l * freq``: ``l * repetition_penalties[i]`` where negative, ``l / repetition_penalties[i]`` where
    positive (unless the penalty is 1); last ``l /= temps[i]`` where ``temps`` and ``temps[i]`` are given.  An fp32 input is
    updated in place and returned; other dtypes return a new tensor in the input dtype."""

    @staticmethod
    def check_call_contract(logits, token_freqs, presence_penalties, frequency_penalties, repetition_penalties, temps):
        if logits.dim() != 2:
            raise ValueError(f"logits must be [B, V], got shape {tuple(logits.shape)}.")
        rows = logits.shape[0]
        for name, seq in (("token_freqs", token_freqs), ("presence_penalties", presence_penalties),
                          ("frequency_penalties", frequency_penalties), ("repetition_penalties", repetition_penalties)):
            if len(seq) != rows:
                raise ValueError(f"{name} has {len(seq)} entries for {rows} rows.")
        if temps is not None and len(temps) != rows:
            raise ValueError(f"temps has {len(temps)} entries for {rows} rows.")
        for f in token_freqs:
            if f is not None and (f.dim() != 1 or f.shape[0] != logits.shape[1]):
                raise ValueError(f"a frequency row must be [V] = [{logits.shape[1]}], got shape {tuple(f.shape)}.")


__all__ = []      # (all six: SAMPLING_OPS, core/operators/__init__.py)
