"""The visibility inputs of tests/visibility.py on the packed layout of `MojoSWA`: contiguous K/V, no pages.

The MAP and SELECTOR families, their expectations (`expected_map`, `expected_selector`: the definition, `window_mask`) and the
comparer are those of `visibility`; only the K/V builder and the selector's plan are new:

* the sequences are adjacent in memory, so a neighbour's keys are the natural poison: in the map family one leaked key changes
  the integer row sum, in the selector a neighbour's key carries the code of ITS position and a probe on every kv head;
* the ``lead`` unused tokens in front of the first sequence and the ``tail`` ones behind the last carry the numeric poison of
  `visibility` (``K[..., 0] = 256``, ``V = 1`` on every channel);
* the selector's edge targets are both sides of every multiple of every stride counted from the SEQUENCE's start and from the
  TENSOR's start (``cu_total_seq_lens[b] + t``): the linear launch is the first form in which the two differ.

Everything here runs on the CPU."""
from dataclasses import dataclass

import torch

from oracle.paged import cu
from visibility import (FAILURES_LISTED, MAP, SELECTOR, Case, Inputs, _dense_k, _dense_v, _own_candidates, bases, compare,
                        expected_map, expected_selector, visible)


@dataclass(frozen=True)
class PackedCase(Case):
    """A `visibility.Case` of kind "prefill" for `MojoSWA`.  ``page`` is 1: the dense builders of `visibility` then make exactly
    ``kv_len`` slots per sequence."""
    lead: int = 5
    tail: int = 7

    def ctor(self):
        return dict(gqa_layout=self.layout, global_window_size=self.glob, local_window_size=self.local)


def packed_case(kv_lens, q_lens, **kw):
    return PackedCase("MojoSWA", "prefill", tuple(kv_lens), tuple(q_lens), page=1, **kw)


class PackedInputs:
    """The tensors of one launch (`visibility.Inputs` without the pages)."""

    def __init__(self, case, family, base=0, targets=None):
        assert case.kind == "prefill" and case.page == 1 and not case.holes
        self.case, self.family, self.base, self.targets = case, family, base, targets
        self._dev, self.dense = {}, {}
        self.cu_q = cu([case.rows(b) for b in range(len(case.kv_lens))])
        self.cu_kv = cu(list(case.kv_lens)) + case.lead
        total = case.lead + sum(case.kv_lens) + case.tail
        k = torch.zeros(total, case.hkv, case.d, dtype=torch.float64)
        for b, n in enumerate(case.kv_lens):
            if n:
                k[int(self.cu_kv[b]): int(self.cu_kv[b + 1])] = _dense_k(case, b, family)[:n]
        k[: case.lead, :, 0] = 256.0
        k[total - case.tail:, :, 0] = 256.0
        self.k = k.to(case.dtype)
        self.set_base(base)
        self.set_targets(targets)

    def set_base(self, base):
        case = self.case
        self.base = base
        self._dev.pop("v", None)
        total = case.lead + sum(case.kv_lens) + case.tail
        v = torch.zeros(total, case.hkv, case.d, dtype=torch.float64)
        for b, n in enumerate(case.kv_lens):
            if n:
                v[int(self.cu_kv[b]): int(self.cu_kv[b + 1])] = _dense_v(case, b, self.family, base)[:n]
        v[: case.lead] = 1.0
        v[total - case.tail:] = 1.0
        self.v = v.to(case.dtype)

    def set_targets(self, targets):
        if self.family == MAP or targets is not None:
            Inputs.set_targets(self, targets)            # (the queries of `visibility`: nothing in them is paged)

    _on = Inputs._on

    def call(self, op, device="cpu"):
        to = lambda name: self._on(name, device)         # noqa: E731
        out = op.forward(to("q"), to("k"), to("v"), to("cu_q"), to("cu_kv"), softmax_scale=1.0)
        return out.detach().cpu()


def _edge_candidates(case, b, strides, start):
    """Both sides of every multiple of every stride, counted from the sequence's start and from the tensor's (``start`` = the
    sequence's first row in K/V), where some row of the sequence sees the key."""
    n = case.kv_lens[b]
    seen = visible(case.rows(b), n, case.local, case.glob).any(dim=0)
    at = set()
    for stride in strides:
        for origin in (0, start):
            first = (-origin) % stride                   # the first key at a multiple of the stride in this count
            at.update(t for m in range(first, n + 1, stride) for t in (m - 1, m) if 0 <= t < n and (m > 0 or origin))
    return [t for t in sorted(at) if bool(seen[t])]


def packed_selector_plan(case, strides):
    """`visibility.selector_plan` with the edge targets of `_edge_candidates` above."""
    span = case.hkv * case.d
    starts = (cu(list(case.kv_lens)) + case.lead).tolist()
    own = [[_own_candidates(case, b, i) for i in range(case.rows(b))] if n > 0 else [] for b, n in enumerate(case.kv_lens)]
    edges = [_edge_candidates(case, b, strides, starts[b]) if n > 0 else [] for b, n in enumerate(case.kv_lens)]
    heads = [case.kv_head(h) for h in range(case.hq)]
    plan = []
    while not plan or any(edges) or any(any(rows) for rows in own):
        base = (len(plan) % case.hkv) * case.d

        def take(waiting, h):
            for j, t in enumerate(waiting):
                if (t - base) % span // case.d == h:
                    return waiting.pop(j)
            return None
        targets = []
        for b, n in enumerate(case.kv_lens):
            t = torch.zeros(case.rows(b), case.hq, dtype=torch.int64)
            for i in range(case.rows(b) if n > 0 else 0):
                for head, h in enumerate(heads):
                    pick = take(own[b][i], h)
                    if pick is None:
                        pick = take(edges[b], h)
                    t[i, head] = max(min(n - case.rows(b) + i, n - 1), 0) if pick is None else pick
            targets.append(t)
        plan.append((base, targets))
        assert len(plan) <= 64, "the selector's plan does not converge"
    return plan


def run_packed_family(case, family, op, device="cpu", strides=(), repeat=False):
    """`visibility.run_family` on the packed layout: ``(failures, worst)`` over every launch of one family."""
    failures, worst = [], 0.0
    if family == MAP:
        inputs = PackedInputs(case, MAP)
        plan = [(base, None) for base in bases(case)]
    else:
        plan = packed_selector_plan(case, strides)
        inputs = PackedInputs(case, SELECTOR, targets=plan[0][1])
    for base, targets in plan:
        inputs.set_base(base)
        if targets is not None:
            inputs.set_targets(targets)
        got = inputs.call(op, device)
        if repeat:
            assert torch.equal(inputs.call(op, device).view(torch.int16), got.view(torch.int16)), "two calls, two results"
        want = expected_map(case, base) if family == MAP else expected_selector(case, inputs)
        f, w = compare(case, inputs, got, want, limit=FAILURES_LISTED)
        failures += f
        worst = max(worst, w)
    return failures, worst
