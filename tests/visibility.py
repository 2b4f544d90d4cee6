"""Inputs on which paged attention returns, exactly, WHICH keys each query row attended.

Two families, one paged-cache builder:

* the visibility map (``MAP``): ``Q[..., 0] = 1``, ``K = 0``, ``softmax_scale = 1``, so every visible key scores 0, ``p = 1`` and
  the row sum is the integer ``n`` whatever the tiling.  ``V`` holds one probe per (kv head, channel): ``V[pos, h, c] = 1`` where
  ``pos == base + h * D + c``.  Output ``[row i, head g of kv head h, channel c]`` is ``[pos visible to row i] / n_i``: exactly 0
  for an invisible probe, ``storage(fp32(1 / n_i))`` within 1 ulp for a visible one.
* the selector (``SELECTOR``): ``K[t]`` carries the +-1 binary code of ``t`` on channels ``1 .. 10``, a query head 16 x the code of
  its target, so scores are exact multiples of 16 and the target leads every other key by >= 32.  ``V`` is the probe tensor with
  positions taken modulo ``Hkv * D``.  A row whose target is visible returns 1.0 on the target's channel; otherwise the expectation
  is the fp64 softmax of the exact scores over the mask.  Targets (`selector_plan`): every row's own causal and window edges, and
  both sides of every multiple of the launch's tile, page, chunk and slice sizes that some row of the sequence sees.

Poison is numbers, never NaN: the slots of a sequence's last page at and past ``kv_len``, and one shared POISON PAGE with a valid
id that every table entry no row can see points at (entries past the last page, whole pages inside a window gap), carry
``K[..., 0] = 256`` (int8: 127) and ``V = 1`` on every channel, so one leaked key takes the whole softmax.  ``-1`` appears only as
the holes of the GQA pair (``Case.holes``): the gather stops at the first negative id, keys behind it count in ``n`` with zero K / V.

Everything here runs on the CPU; the expected values come from the definition (`visible`), not from a golden.
"""
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from oracle.paged import cu, window_mask

MAP, SELECTOR = "map", "selector"
CODE_BITS = 10                       # positions below 1024
SELECTOR_TOL = {torch.bfloat16: 2.0 ** -5, torch.float16: 2.0 ** -8}      # 4 ulp of the storage type at 1.0
FAILURES_LISTED = 64                 # per sequence and launch in `run_family` (a broken kernel fails everywhere)
INT8_OPS = ("MojoPagedDecodeGQAWithKVDequant", "MojoPagedPrefillGQAWithKVDequant", "MojoPagedDecodeSWAWithKVDequant",
            "MojoPagedPrefillSWAWithKVDequant", "MojoPagedDecodeNstepSWAWithKVDequant")
WINDOW_OPS = ("MojoPagedDecodeSWA", "MojoPagedPrefillSWA", "MojoPagedDecodeNstepSWA", "MojoPagedDecodeSWAWithKVDequant",
              "MojoPagedPrefillSWAWithKVDequant", "MojoPagedDecodeNstepSWAWithKVDequant")


@dataclass(frozen=True)
class Case:
    """One geometry.  ``kind``: "decode" (one row per sequence, ``[B, Hq, D]``), "nstep" (``steps`` rows, ``[B, S, Hq, D]``) or
    "prefill" (``q_lens[b]`` rows, packed ``[T, Hq, D]`` with ``pad_tokens`` rows of padding behind the last sequence).
    ``holes``: ``(sequence, logical page)`` table entries set to -1 (GQA pair only)."""
    op: str
    kind: str
    kv_lens: Tuple[int, ...]
    q_lens: Optional[Tuple[int, ...]] = None
    steps: int = 1
    hq: int = 8
    hkv: int = 2
    d: int = 128
    page: int = 16
    dtype: torch.dtype = torch.bfloat16
    layout: str = "AABB"
    local: Optional[int] = None
    glob: Optional[int] = None
    holes: Tuple[Tuple[int, int], ...] = ()
    pad_tokens: int = 0
    seed: int = 0

    @property
    def int8(self):
        return self.op in INT8_OPS

    @property
    def group(self):
        return self.hq // self.hkv

    def rows(self, b):
        return {"decode": 1, "nstep": self.steps}.get(self.kind) or self.q_lens[b]

    def kv_head(self, head):
        return head // self.group if self.layout == "AABB" else head % self.hkv

    def valid_len(self, b):
        """Keys in front of the sequence's first hole (all of them without one)."""
        first = min((p for s, p in self.holes if s == b), default=None)
        return self.kv_lens[b] if first is None else min(self.kv_lens[b], first * self.page)

    def ctor(self):
        kw = dict(gqa_layout=self.layout)
        if self.op in WINDOW_OPS:
            kw.update(global_window_size=self.glob, local_window_size=self.local)
        else:
            assert self.local is None and self.glob is None
        return kw

    def make(self, cls):
        op = cls(**self.ctor())
        if self.int8:
            op.query_dtype = self.dtype          # (the constructor admits bf16 only; the forward's math is dtype-generic)
        return op


def visible(q_len, kv_len, local, glob):
    """``[q_len, kv_len]`` bool: the definition, `oracle.paged.window_mask` (row i at position ``kv_len - q_len + i``)."""
    return window_mask(q_len, kv_len, local, glob)


def bases(case):
    """Probe offsets of the map family that cover every key position of every sequence."""
    span = case.hkv * case.d
    return [i * span for i in range(max(1, -(-max(case.kv_lens) // span)))]


def code(pos):
    """``[..., CODE_BITS]`` of +-1.0: the binary code of int64 positions."""
    bits = (pos.unsqueeze(-1) >> torch.arange(CODE_BITS)) & 1
    return (2 * bits - 1).to(torch.float64)


# ---- the paged cache --------------------------------------------------------------------------------------------------
def _seq_pages(case, b):
    return -(-case.kv_lens[b] // case.page)


def _gap_pages(case, b):
    """Logical pages of sequence b that hold no key any of its rows sees."""
    n = case.kv_lens[b]
    seen = visible(case.rows(b), n, case.local, case.glob).any(dim=0)
    return [p for p in range(_seq_pages(case, b)) if not bool(seen[p * case.page:(p + 1) * case.page].any())]


def _dense_k(case, b, family):
    """``[pages * page, Hkv, D]`` fp64: zero (map) or the position code on channels 1.. (selector); poison behind ``kv_len``."""
    n, slots = case.kv_lens[b], _seq_pages(case, b) * case.page
    k = torch.zeros(slots, case.hkv, case.d, dtype=torch.float64)
    if family == SELECTOR:
        assert n <= 1 << CODE_BITS and case.d > CODE_BITS
        k[:n, :, 1:1 + CODE_BITS] = code(torch.arange(n)).unsqueeze(1)
    k[n:, :, 0] = 127.0 if case.int8 else 256.0
    return k


def _dense_v(case, b, family, base):
    """``[pages * page, Hkv, D]`` fp64: the probes (selector: positions modulo ``Hkv * D``); all ones behind ``kv_len``."""
    n, slots, span = case.kv_lens[b], _seq_pages(case, b) * case.page, case.hkv * case.d
    idx = torch.arange(slots) - base
    if family == SELECTOR:
        idx = idx % span
    hit = (idx >= 0) & (idx < span)
    v = torch.zeros(slots, span, dtype=torch.float64)
    v[torch.arange(slots)[hit], idx[hit]] = 1.0
    v[n:] = 1.0
    return v.view(slots, case.hkv, case.d)


def _store(cache, ids, dense, case):
    pages = dense.view(len(ids), case.page, case.hkv, case.d).permute(0, 2, 1, 3)
    cache[torch.tensor(ids, dtype=torch.int64)] = pages.to(cache.dtype)


class Inputs:
    """The tensors of one launch and how to hand them to an operator (hip or golden)."""

    def __init__(self, case, family, base=0, targets=None):
        self.case, self.family, self.base, self.targets = case, family, base, targets
        self._dev, self._probes, self.dense = {}, [], {}
        g = torch.Generator().manual_seed(case.seed)
        need = [_seq_pages(case, b) for b in range(len(case.kv_lens))]
        total = sum(need) + 3
        perm = torch.randperm(total, generator=g).tolist()                      # random placement of the pages
        self.poison = perm[0]
        cdt = torch.int8 if case.int8 else case.dtype
        self.k = torch.zeros(total, case.hkv, case.page, case.d, dtype=cdt)
        self.v = torch.zeros(total, case.hkv, case.page, case.d, dtype=cdt)
        vq = 64.0 if case.int8 else 1.0                                         # int8: 64 * value_scale 2^-6 = 1
        for spare in perm[:3]:                                                  # the poison page (and two unreferenced ones)
            self.k[spare, :, :, 0] = 127 if case.int8 else 256
            self.v[spare] = vq
        self.table = torch.full((len(need), max(max(need), 1)), self.poison, dtype=torch.int32)
        self.ids, at = [], 3
        for b, n_pages in enumerate(need):
            ids = perm[at:at + n_pages]
            at += n_pages
            self.ids.append(ids)
            if n_pages:
                _store(self.k, ids, _dense_k(case, b, family), case)
                tail = torch.zeros(n_pages * case.page, case.hkv, case.d, dtype=torch.float64)
                tail[case.kv_lens[b]:] = vq                                      # the slots behind the last key: V = 1
                _store(self.v, ids, tail, case)
                self.table[b, :n_pages] = torch.tensor(ids, dtype=torch.int32)
                for p in _gap_pages(case, b):
                    self.table[b, p] = self.poison
        for b, p in case.holes:
            assert case.op in ("MojoPagedDecodeGQA", "MojoPagedPrefillGQA") and 0 < p < need[b]
            self.table[b, p] = -1
        self.set_base(base)
        if case.int8:
            self.ks = torch.ones(case.hkv, case.d, dtype=torch.bfloat16)
            self.vs = torch.full((case.hkv, case.d), 2.0 ** -6, dtype=torch.bfloat16)
        self.lens = torch.tensor(case.kv_lens, dtype=torch.int32)
        n_rows = [case.rows(b) for b in range(len(need))]
        self.cu_q, self.cu_kv = cu(n_rows), cu(list(case.kv_lens))
        self.set_targets(targets)

    def set_base(self, base):
        """(Re)write the probes for another offset; K, the table and the queries stay."""
        case, vq = self.case, (64 if self.case.int8 else 1)
        for at in self._probes:                                                  # take the old probes out, put the new ones in
            self.v[at] = 0
        self.base, self._probes = base, []
        self._dev.pop("v", None)
        span = case.hkv * case.d
        for b, ids in enumerate(self.ids):
            pos = torch.arange(case.kv_lens[b])
            idx = (pos - base) % span if self.family == SELECTOR else pos - base
            pos, idx = pos[(idx >= 0) & (idx < span)], idx[(idx >= 0) & (idx < span)]
            if pos.numel():
                at = (torch.tensor(ids)[pos // case.page], idx // case.d, pos % case.page, idx % case.d)
                self.v[at] = vq
                self._probes.append(at)

    def set_targets(self, targets):
        """Queries: ``Q[..., 0] = 1`` (map); ``Q[..., 0] = 2`` and 16 x the code of ``targets[b][row, head]`` (selector)."""
        case = self.case
        self.targets = targets
        self._dev.pop("q", None)
        per_seq = []
        for b in range(len(case.kv_lens)):
            q = torch.zeros(case.rows(b), case.hq, case.d, dtype=torch.float64)
            if self.family == MAP:
                q[..., 0] = 1.0
            else:
                q[..., 0] = 2.0              # poison (256, int8 127) then outscores the best code score, 160
                q[..., 1:1 + CODE_BITS] = 16.0 * code(targets[b])
            per_seq.append(q)
        self.q64 = per_seq
        self.q = pack(case, [q.to(case.dtype) for q in per_seq])

    def _on(self, name, device):
        """Tensor ``name`` on ``device``; the copy is kept until `set_base` / `set_targets` rewrite the tensor."""
        if device == "cpu":
            return getattr(self, name)
        if self._dev.get(name) is None or self._dev[name][0] != device:
            self._dev[name] = (device, getattr(self, name).to(device))
        return self._dev[name][1]

    def call(self, op, device="cpu"):
        """Run ``op`` (``softmax_scale = 1.0``, no hint) and return its output on the CPU."""
        case = self.case
        to = lambda name: self._on(name, device)                                 # noqa: E731
        caches = (None, to("k"), to("ks"), to("v"), to("vs")) if case.int8 else (to("k"), to("v"))
        if case.kind == "prefill":
            out = op.forward(to("q"), *caches, to("cu_q"), to("table"), softmax_scale=1.0, cu_total_seq_lens=to("cu_kv"))
        else:
            out = op.forward(to("q"), *caches, to("lens"), to("table"), softmax_scale=1.0)
        return out.detach().cpu()


def pack(case, per_seq):
    """Per-sequence ``[rows, Hq, D]`` tensors in the operator's layout."""
    if case.kind == "decode":
        return torch.stack([x[0] for x in per_seq])
    if case.kind == "nstep":
        return torch.stack(per_seq)
    pad = torch.zeros(case.pad_tokens, case.hq, case.d, dtype=per_seq[0].dtype)
    return torch.cat(list(per_seq) + [pad])


def unpack(case, out):
    """The inverse of `pack`; a prefill's padding rows come back as one more entry."""
    if case.kind == "decode":
        return [out[b:b + 1] for b in range(out.shape[0])]
    if case.kind == "nstep":
        return [out[b] for b in range(out.shape[0])]
    edges = cu([case.rows(b) for b in range(len(case.kv_lens))]).tolist()
    return [out[lo:hi] for lo, hi in zip(edges[:-1], edges[1:])] + [out[edges[-1]:]]


# ---- targets of the selector -----------------------------------------------------------------------------------------
def _own_candidates(case, b, row):
    """The edges of ONE row: its first and last visible key, ``lo``, ``lo - 1``, ``p + 1``, ``glob - 1``, ``glob`` and the
    sequence's last key."""
    n = case.kv_lens[b]
    p = n - case.rows(b) + row
    lo = max(p - case.local, 0) if case.local is not None else 0
    want = [p, p + 1, lo, lo - 1, 0, n - 1]
    if case.glob is not None:
        want += [case.glob - 1, case.glob]
    return list(dict.fromkeys(t for t in want if 0 <= t < n))


def _edge_candidates(case, b, strides):
    """Both sides of EVERY multiple of every stride (tile, page, chunk, slice of the launch) below the sequence's length, where
    some row of the sequence sees the key: a launch walks the tiles of its visible ranges only, and the keys just outside a
    window are each row's own candidates."""
    n = case.kv_lens[b]
    seen = visible(case.rows(b), n, case.local, case.glob).any(dim=0)
    at = sorted({t for stride in strides for m in range(stride, n, stride) for t in (m - 1, m)})
    return [t for t in at if bool(seen[t])]


def selector_plan(case, strides):
    """The launches of the selector family: ``[(base, targets)]``, ``targets[b]`` int64 ``[rows, Hq]``.

    A target shows as 1.0 only under a query head whose kv head holds its probe — kv head ``((t - base) % (Hkv * D)) // D`` —
    so every (row, head) slot takes the next waiting candidate of ITS kv head: first the row's own edges, then the sequence's
    tile / page / chunk / slice edges, which the rows of a sequence share between them.  Launches go on, the probe offset moving
    by ``D`` each time, until every candidate of every row and sequence has met a head; a slot with nothing waiting repeats the
    row's last key."""
    span = case.hkv * case.d
    own = [[_own_candidates(case, b, i) for i in range(case.rows(b))] if n > 0 else [] for b, n in enumerate(case.kv_lens)]
    edges = [_edge_candidates(case, b, strides) if n > 0 else [] for b, n in enumerate(case.kv_lens)]
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
    return plan


# ---- expectations -----------------------------------------------------------------------------------------------------
def expected_map(case, base):
    """Per sequence ``[rows, Hq, D]`` in the storage type: ``storage(fp32(1 / n_i))`` where the probed position is visible to
    the row and in front of the first hole, exact 0 elsewhere (rows that see no key: zeros)."""
    out = []
    heads = torch.tensor([case.kv_head(h) for h in range(case.hq)])
    pos = base + heads[:, None] * case.d + torch.arange(case.d)[None, :]            # [Hq, D] probed positions
    for b, n in enumerate(case.kv_lens):
        rows = case.rows(b)
        mask = visible(rows, n, case.local, case.glob)                              # [rows, n]
        count = mask.sum(dim=1)
        live = mask.clone()
        live[:, case.valid_len(b):] = False
        hit = torch.zeros(rows, case.hq, case.d, dtype=torch.bool)
        ok = pos < n
        hit[:, ok] = live[:, pos[ok]]
        share = (torch.ones(rows, dtype=torch.float32) / count.clamp(min=1).to(torch.float32)).to(case.dtype)
        out.append(torch.where(hit, share[:, None, None], torch.zeros((), dtype=case.dtype)))
    if case.kind == "prefill":
        out.append(torch.zeros(case.pad_tokens, case.hq, case.d, dtype=case.dtype))
    return out


def expected_selector(case, inputs):
    """Per sequence ``[rows, Hq, D]`` fp64: the softmax of the exact scores over `visible`, times the probes."""
    out = []
    for b, n in enumerate(case.kv_lens):
        rows, valid = case.rows(b), case.valid_len(b)
        if n == 0:
            out.append(torch.zeros(rows, case.hq, case.d, dtype=torch.float64))
            continue
        if (b, inputs.base) not in inputs.dense:                                    # (the same for every launch at this offset)
            k = _dense_k(case, b, SELECTOR)[:n, 0]                                  # [n, D] (the same for every kv head)
            v = _dense_v(case, b, SELECTOR, inputs.base)[:n]                        # [n, Hkv, D]
            k[valid:] = 0.0
            v[valid:] = 0.0
            inputs.dense[b, inputs.base] = (k, v[:, [case.kv_head(h) for h in range(case.hq)]])       # [n, Hq, D]
        k, v_q = inputs.dense[b, inputs.base]
        s = torch.einsum("rhd,nd->rhn", inputs.q64[b], k)
        mask = visible(rows, n, case.local, case.glob)[:, None, :]
        s = torch.where(mask, s, float("-inf"))
        w = torch.softmax(s, dim=-1)
        w = torch.where(mask.any(dim=-1, keepdim=True), w, torch.zeros((), dtype=torch.float64))    # rows that see no key
        out.append(torch.einsum("rhn,nhd->rhd", w, v_q))
    if case.kind == "prefill":
        out.append(torch.zeros(case.pad_tokens, case.hq, case.d, dtype=torch.float64))
    return out


# ---- the comparer -----------------------------------------------------------------------------------------------------
def _ordinal(x):
    """16-bit floats as integers that step by one per representable value (sign-magnitude -> two's complement)."""
    bits = x.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(bits < 0, -(bits & 0x7FFF), bits)


def compare(case, inputs, got, want, limit=None):
    """``(failures, worst)``: per failing element ``(sequence, row, q head, probed key position, got, want)`` (sequence
    ``len(kv_lens)``: the padding rows; at most ``limit`` per sequence), and the worst deviation — in ulp of the storage type
    (map) or absolute (selector).

    Map: a ``want`` of 0 must read exactly 0, any other within 1 ulp.  Selector: within `SELECTOR_TOL`."""
    failures, worst = [], 0.0
    span = case.hkv * case.d
    for b, (g, w) in enumerate(zip(unpack(case, got), want)):
        assert g.shape == w.shape and g.dtype == case.dtype, (g.shape, w.shape, g.dtype)
        if g.numel() == 0:
            continue
        if inputs.family == MAP:
            err = (_ordinal(g) - _ordinal(w)).abs().to(torch.float64)
            err = torch.where(torch.isfinite(g.float()), err, torch.full_like(err, float("inf")))
            bad = torch.where(w == 0, g != 0, err > 1)
            err = torch.where((w == 0) & (g != 0), err.clamp(min=2.0), err)
        else:
            err = (g.double() - w).abs()
            err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
            bad = err > SELECTOR_TOL[case.dtype]
        worst = max(worst, float(err.max()))
        for row, head, c in bad.nonzero()[:limit].tolist():
            pos = inputs.base + case.kv_head(head) * case.d + c
            if inputs.family == SELECTOR and b < len(case.kv_lens):                 # the position this channel stands for
                t = int(inputs.targets[b][row, head])
                pos = t if (t - inputs.base) % span == case.kv_head(head) * case.d + c else pos
            failures.append((b, row, head, pos, float(g[row, head, c]), float(w[row, head, c])))
    return failures, worst


def report(failures, limit=12):
    lines = [f"seq {b} row {r} head {h} key {p}: got {g!r} want {w!r}" for b, r, h, p, g, w in failures[:limit]]
    return f"{len(failures)} elements differ\n" + "\n".join(lines)


def run_family(case, family, op, device="cpu", strides=(), repeat=False):
    """Every launch of one family through ``op``; returns ``(failures, worst)`` over all of them.  ``strides``: the tile, page,
    chunk and slice sizes of the launch (`selector_plan`).  ``repeat``: each call is made twice and must return the same bits."""
    failures, worst = [], 0.0
    if family == MAP:
        inputs = Inputs(case, MAP)
        plan = [(base, None) for base in bases(case)]
    else:
        plan = selector_plan(case, strides)
        inputs = Inputs(case, SELECTOR, targets=plan[0][1])
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
