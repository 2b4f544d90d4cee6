"""The exact-answer inputs of tests/visibility.py in the MLA data layout: which keys did each row attend?

The MLA pair reads a latent cache ``c [N, 1, page, r]`` and a rope cache ``k_pe [N, 1, page, rope]``; ``kv_b_proj`` viewed as
``[H, nope + vd, r]`` decompresses the latent into ``K_nope`` (rows ``:nope``, W_k) and ``V`` (rows ``nope:``, W_v).  Every launch
runs with ``softmax_scale = 1.0``.  Three families:

* the visibility map (``MAP``): ``q_nope = 0``, ``q_rope[..., 0] = 1``, ``k_pe = 0`` on live keys, so every visible key scores 0.
  The latent of key ``s`` is one-hot, ``c[s] = e_{s - base}`` (zero where ``s - base`` falls outside ``[0, r)``), W_k is zero and
  ``W_v[h][c, j] = 1`` iff ``j == (h * vd + c) % r``: ``out[row, h, c] = [key base + (h * vd + c) % r visible to row] / n_row``,
  exactly 0 for an invisible probe and ``storage(fp32(1 / n))`` within 1 ulp for a visible one.  ``base`` steps by
  ``min(r, H * vd)`` until every key of every sequence was probed.  With ``Case.sink`` the sink logit is 0.0 on even heads and
  -30000.0 on odd ones: the denominators are ``n + 1`` and ``n``, both exact — a sink added once per key split, left out, or
  indexed by the wrong head shows.
* the rope-coded selector (``SEL_ROPE``): ``k_pe[s, 1 .. bits] = code(s)``, ``q_rope[1 .. bits] = 16 * code(target)``; the probes
  sit in the latent as above, positions modulo ``r``.  The target leads every other key by >= 32, so the row returns 1.0 on the
  target's channel: ``k_pe`` row ``s`` must have met latent row ``s`` (every kernel stages the two as separate LDS images).
* the nope-coded selector (``SEL_NOPE``): the code rides the latent on its last 16 channels, ``W_k[h][d, r - 16 + d] = 1`` for
  ``d < bits`` and ``q_nope[:bits] = 16 * code(target)``; the probes sit on the first ``r - 16`` channels (W_v is zero on the code
  channels; positions modulo ``r - 16``).  This pins the absorbed query GEMM, or the decompressed ``K_nope``, per head.

Poison is numbers: the slots of a sequence's last page at and past ``kv_len``, and one shared poison page with a valid id that
stands in every table entry behind the last page, hold ``k_pe[..., 0] = 256`` and ``c = 1`` on every probe channel; the queries
carry ``q_rope[..., 0] = 1`` (map) or ``2`` (selectors, 512 against a best code score of ``16 * bits <= 208``), so one leaked key
takes the whole softmax.  ``-1`` appears only as ``Case.holes`` (decode, logical page >= 1).

The expectation is the definition: a row at position ``kv_len - q_len + i`` sees keys ``0 .. position``, cut at the first hole.
Unlike the GQA pair, keys behind a hole do NOT count in ``n`` (the goldens drop the tail: `oracle.torch_golden._mla_unpage`).  A
row with no key reads zeros, and so do padding rows.  Everything here runs on the CPU and calls no golden."""
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

import visibility as V
from visibility import SELECTOR_TOL, _ordinal, cu, report  # noqa: F401  (re-exported for the tests)

MAP, SEL_ROPE, SEL_NOPE = "map", "selector:rope", "selector:nope"
FAMILIES = (MAP, SEL_ROPE, SEL_NOPE)
CODE_CHANNELS = 16                   # latent channels the nope-coded selector keeps for the code
FAILURES_LISTED = 64
SINK_ON, SINK_OFF = 0.0, -30000.0    # even / odd heads


# ---- sizes, as the host code computes them (csrc/mla_attn.hip: mla_plan) ------------------------------------------------
def default_splits(tokens, heads, r, rope, capacity):
    """`mla_splits` without the switch: 256 workgroups' worth of splits, at most one per 256 keys of the capacity, 1 .. 64."""
    tiles = tokens * ((heads + 63) // 64 if (r, rope) == (512, 64) else 1)
    return max(1, min(256 // max(tiles, 1), -(-capacity // 256), 64))


def split_keys(capacity, splits):
    return -(-(-(-capacity // splits)) // 64) * 64


@dataclass(frozen=True)
class Case:
    """One geometry.  ``kind``: "decode" (one row per sequence, ``[B, H, nope + rope]``) or "prefill" (``q_lens[b]`` rows, packed,
    ``pad_tokens`` rows of padding behind the last sequence).  ``holes``: ``(sequence, logical page >= 1)`` table entries set
    to -1 (decode only).  ``table_pages``: the least width of the block table (its capacity sizes the key splits)."""
    op: str
    kind: str
    kv_lens: Tuple[int, ...]
    q_lens: Optional[Tuple[int, ...]] = None
    heads: int = 8
    nope: int = 64
    rope: int = 32
    vd: int = 64
    r: int = 32
    page: int = 16
    dtype: torch.dtype = torch.bfloat16
    sink: bool = False
    holes: Tuple[Tuple[int, int], ...] = ()
    pad_tokens: int = 0
    seed: int = 0
    code_bits: int = V.CODE_BITS
    table_pages: int = 0

    def rows(self, b):
        return 1 if self.kind == "decode" else self.q_lens[b]

    def valid_len(self, b):
        """Keys in front of the sequence's first hole (all of them without one)."""
        first = min((p for s, p in self.holes if s == b), default=None)
        return self.kv_lens[b] if first is None else min(self.kv_lens[b], first * self.page)

    def counts(self, b):
        """``[rows]`` int64: the number of keys each row of sequence b sees."""
        n, rows = self.kv_lens[b], self.rows(b)
        return (torch.arange(rows) + (n - rows + 1)).clamp(min=0, max=self.valid_len(b))

    def span(self, family):
        """Latent channels that hold probes."""
        return self.r - CODE_CHANNELS if family == SEL_NOPE else self.r

    def make(self, cls, device="cpu"):
        kw = dict(use_attn_sink=self.sink)
        if self.kind == "prefill":
            kw["is_causal"] = True
        return cls(self.heads, self.nope, self.rope, self.vd, self.r, **kw).to(self.dtype).to(device)


def code(pos, bits=V.CODE_BITS):
    """``[..., bits]`` of +-1.0: the binary code of int64 positions (`visibility.code` at its own width)."""
    if bits == V.CODE_BITS:
        return V.code(pos)
    return (2 * ((pos.unsqueeze(-1) >> torch.arange(bits)) & 1) - 1).to(torch.float64)


def probe_index(case, family):
    """``[H, vd]`` int64: the latent channel that output ``[h, c]`` reads."""
    return (torch.arange(case.heads)[:, None] * case.vd + torch.arange(case.vd)[None, :]) % case.span(family)


def weights(case, family):
    """``kv_b_proj`` as ``[H, nope + vd, r]`` fp64."""
    w = torch.zeros(case.heads, case.nope + case.vd, case.r, dtype=torch.float64)
    j = probe_index(case, family)
    h, c = torch.meshgrid(torch.arange(case.heads), torch.arange(case.vd), indexing="ij")
    w[h, case.nope + c, j] = 1.0
    if family == SEL_NOPE:
        assert case.code_bits <= min(CODE_CHANNELS, case.nope) and case.r > CODE_CHANNELS
        d = torch.arange(case.code_bits)
        w[:, d, case.r - CODE_CHANNELS + d] = 1.0
    return w


def sink_logits(case):
    if not case.sink:
        return None
    return torch.where(torch.arange(case.heads) % 2 == 0, SINK_ON, SINK_OFF).to(torch.float32)


def bases(case):
    """Probe offsets of the map family that cover every key position of every sequence."""
    step = min(case.r, case.heads * case.vd)
    return [i * step for i in range(max(1, -(-max(case.kv_lens) // step)))]


# ---- the paged caches -------------------------------------------------------------------------------------------------
def _seq_pages(case, b):
    return -(-case.kv_lens[b] // case.page)


def _dense_latent(case, b, family, base):
    """``[pages * page, r]`` fp64: the probes (selectors: positions modulo the span, and the code of the nope-coded one); ones on
    every probe channel behind ``kv_len``."""
    n, slots, span = case.kv_lens[b], _seq_pages(case, b) * case.page, case.span(family)
    pos = torch.arange(slots)
    idx = pos - base if family == MAP else (pos - base) % span
    hit = (idx >= 0) & (idx < span)
    c = torch.zeros(slots, case.r, dtype=torch.float64)
    c[pos[hit], idx[hit]] = 1.0
    if family == SEL_NOPE:
        c[:, case.r - CODE_CHANNELS:case.r - CODE_CHANNELS + case.code_bits] = code(pos, case.code_bits)
    c[n:] = 0.0
    c[n:, :span] = 1.0
    return c


def _dense_kpe(case, b, family):
    """``[pages * page, rope]`` fp64: zero, or the position code on channels 1.. (rope-coded selector); poison behind ``kv_len``."""
    n, slots = case.kv_lens[b], _seq_pages(case, b) * case.page
    k = torch.zeros(slots, case.rope, dtype=torch.float64)
    if family == SEL_ROPE:
        assert n <= 1 << case.code_bits and case.rope > case.code_bits
        k[:, 1:1 + case.code_bits] = code(torch.arange(slots), case.code_bits)
    k[n:] = 0.0
    k[n:, 0] = 256.0
    return k


class Inputs:
    """The tensors of one launch and how to hand them to an operator (hip or golden)."""

    def __init__(self, case, family, base=0, targets=None):
        assert family in FAMILIES and (case.kind == "decode" or not case.holes)
        assert family != SEL_NOPE or max(case.kv_lens) <= 1 << case.code_bits
        self.case, self.family = case, family
        self._dev = {}
        g = torch.Generator().manual_seed(case.seed)
        need = [_seq_pages(case, b) for b in range(len(case.kv_lens))]
        total = sum(need) + 3
        perm = torch.randperm(total, generator=g).tolist()                      # random placement of the pages
        self.poison, self.zero_page = perm[0], perm[1]                          # (the zero page: no table names it)
        self.ckv = torch.zeros(total, 1, case.page, case.r, dtype=case.dtype)
        self.kpe = torch.zeros(total, 1, case.page, case.rope, dtype=case.dtype)
        for spare in (perm[0], perm[2]):                                         # the poison page (and an unreferenced one)
            self.kpe[spare, :, :, 0] = 256
            self.ckv[spare, :, :, :case.span(family)] = 1
        self.table = torch.full((len(need), max(max(need), case.table_pages, 1)), self.poison, dtype=torch.int32)
        self.ids, at = [], 3
        for b, n_pages in enumerate(need):
            ids = perm[at:at + n_pages]
            at += n_pages
            self.ids.append(torch.tensor(ids, dtype=torch.int64))
            if n_pages:
                self.kpe[self.ids[b], 0] = _dense_kpe(case, b, family).view(n_pages, case.page, case.rope).to(case.dtype)
                self.table[b, :n_pages] = torch.tensor(ids, dtype=torch.int32)
        self.whole_table = self.table.clone()                                    # (before the holes: for the wrong goldens)
        for b, p in case.holes:
            assert 0 < p < need[b]
            self.table[b, p] = -1
        self.w = weights(case, family).view(-1, case.r).to(case.dtype)
        self.sink = sink_logits(case)
        self.lens = torch.tensor(case.kv_lens, dtype=torch.int32)
        n_rows = [case.rows(b) for b in range(len(need))]
        self.cu_q, self.cu_kv = cu(n_rows), cu(list(case.kv_lens))
        self.set_base(base)
        self.set_targets(targets)

    def set_base(self, base):
        """(Re)write the latent for another probe offset; k_pe, the table and the queries stay."""
        case = self.case
        self.base = base
        self._dev.pop("ckv", None)
        for b, ids in enumerate(self.ids):
            if len(ids):
                self.ckv[ids, 0] = _dense_latent(case, b, self.family, base).view(len(ids), case.page, case.r).to(case.dtype)

    def set_targets(self, targets):
        """Queries: ``q_rope[..., 0] = 1`` (map); ``2`` and 16 x the code of ``targets[b][row, head]`` (selectors)."""
        case, bits = self.case, self.case.code_bits
        self.targets = targets
        self._dev.pop("q", None)
        per_seq = []
        for b in range(len(case.kv_lens)):
            q = torch.zeros(case.rows(b), case.heads, case.nope + case.rope, dtype=torch.float64)
            if self.family == MAP:
                q[..., case.nope] = 1.0
            else:
                q[..., case.nope] = 2.0
                at = case.nope + 1 if self.family == SEL_ROPE else 0
                q[..., at:at + bits] = 16.0 * code(targets[b], bits)
            per_seq.append(q)
        self.q64 = per_seq
        self.q = pack(case, [q.to(case.dtype) for q in per_seq])

    def _on(self, name, device):
        if device == "cpu":
            return getattr(self, name)
        if self._dev.get(name) is None or self._dev[name][0] != device:
            self._dev[name] = (device, getattr(self, name).to(device))
        return self._dev[name][1]

    def load(self, op):
        """This family's ``kv_b_proj`` and sink logits into ``op`` (a version-bumping copy)."""
        if getattr(op, "_visibility_weights", None) != (id(self), self.family):
            with torch.no_grad():
                op.kv_b_proj.copy_(self.w)
                if self.case.sink:
                    op.attn_sink.copy_(self.sink)
            op._visibility_weights = (id(self), self.family)

    def call(self, op, device="cpu", no_cu_kv=False, **kw):
        """Run ``op`` (``softmax_scale = 1.0``; ``kw``: the hip classes' keyword extensions) and return its output on the CPU.
        ``no_cu_kv``: the prefill's ``cu_total_seq_lens=None`` form (every sequence's keys are its queries)."""
        case = self.case
        to = lambda name: self._on(name, device)                                 # noqa: E731
        self.load(op)
        if case.kind == "prefill":
            assert not no_cu_kv or tuple(case.q_lens) == tuple(case.kv_lens)
            out = op.forward(to("q"), to("ckv"), to("kpe"), to("cu_q"), to("table"), softmax_scale=1.0,
                             cu_total_seq_lens=None if no_cu_kv else to("cu_kv"), **kw)
        else:
            out = op.forward(to("q"), to("ckv"), to("kpe"), to("lens"), to("table"), softmax_scale=1.0, **kw)
        return out.detach().cpu()


def pack(case, per_seq):
    """Per-sequence ``[rows, H, X]`` tensors in the operator's layout."""
    if case.kind == "decode":
        return torch.stack([x[0] for x in per_seq])
    pad = torch.zeros(case.pad_tokens, *per_seq[0].shape[1:], dtype=per_seq[0].dtype)
    return torch.cat(list(per_seq) + [pad])


def unpack(case, out):
    """The inverse of `pack`; a prefill's padding rows come back as one more entry."""
    if case.kind == "decode":
        return [out[b:b + 1] for b in range(out.shape[0])]
    edges = cu([case.rows(b) for b in range(len(case.kv_lens))]).tolist()
    return [out[lo:hi] for lo, hi in zip(edges[:-1], edges[1:])] + [out[edges[-1]:]]


# ---- targets of the selectors -----------------------------------------------------------------------------------------
def own_candidates(case, b, row):
    """The edges of ONE row: its last visible key ``p``, ``p + 1``, key 0, the sequence's last key, and both sides of the
    sequence's first hole."""
    n = case.kv_lens[b]
    p = n - case.rows(b) + row
    want = [p, p + 1, 0, n - 1]
    if case.valid_len(b) < n:
        want += [case.valid_len(b) - 1, case.valid_len(b)]
    return list(dict.fromkeys(t for t in want if 0 <= t < n))


def edge_candidates(case, b, strides, extra=()):
    """Both sides of EVERY multiple of every stride (tile, split, page of the launch) that some row of the sequence sees, and
    the positions of ``extra`` (both sides of a boundary named by the caller) that it sees."""
    n, valid = case.kv_lens[b], case.valid_len(b)
    at = {t for stride in strides for m in range(stride, n, stride) for t in (m - 1, m)} | set(extra)
    return [t for t in sorted(at) if 0 <= t < valid]


def selector_plan(case, family, strides, extra=()):
    """The launches of a selector family: ``[(base, targets)]``, ``targets[b]`` int64 ``[rows, H]``.

    A target ``t`` shows as 1.0 only under a head whose ``vd`` probe indices contain ``(t - base) % span``, so every (row, head)
    slot takes the next waiting candidate it can show: first the row's own edges, then the sequence's stride edges, which the
    rows of a sequence share between them.  Launches go on, the probe offset moving by ``vd`` each time, until every candidate
    has met such a head; a slot with nothing waiting repeats the row's last key."""
    span = case.span(family)
    shows = torch.zeros(case.heads, span, dtype=torch.bool)
    shows[torch.arange(case.heads)[:, None], probe_index(case, family)] = True
    shows = shows.tolist()
    own = [[own_candidates(case, b, i) for i in range(case.rows(b))] if n > 0 else [] for b, n in enumerate(case.kv_lens)]
    edges = [edge_candidates(case, b, strides, extra) if n > 0 else [] for b, n in enumerate(case.kv_lens)]
    plan = []
    while not plan or any(edges) or any(any(rows) for rows in own):
        base = (len(plan) * case.vd) % span
        assert len(plan) < 4096

        def take(waiting, h):
            for j, t in enumerate(waiting):
                if shows[h][(t - base) % span]:
                    return waiting.pop(j)
            return None
        targets = []
        for b, n in enumerate(case.kv_lens):
            t = torch.zeros(case.rows(b), case.heads, dtype=torch.int64)
            for i in range(case.rows(b) if n > 0 else 0):
                last = max(min(n - case.rows(b) + i, n - 1), 0)
                if not own[b][i] and not edges[b]:
                    t[i] = last
                    continue
                for h in range(case.heads):
                    pick = take(own[b][i], h)
                    if pick is None:
                        pick = take(edges[b], h)
                    t[i, h] = last if pick is None else pick
            targets.append(t)
        plan.append((base, targets))
    return plan


# ---- expectations -----------------------------------------------------------------------------------------------------
def _denominators(case, b):
    """``[rows, H]`` fp64: the visible keys of each row, plus one on the heads whose sink logit is 0."""
    den = case.counts(b).to(torch.float64)[:, None].expand(-1, case.heads).clone()
    if case.sink:
        den[:, 0::2] += 1.0
    return den


def expected_map(case, base):
    """Per sequence ``[rows, H, vd]`` in the storage type: ``storage(fp32(1 / den))`` where the probed key is visible to the row,
    exact 0 elsewhere (rows that see no key: zeros)."""
    out = []
    pos = base + probe_index(case, MAP)                                             # [H, vd] probed positions
    for b in range(len(case.kv_lens)):
        count = case.counts(b)
        hit = pos[None] < count[:, None, None]                                      # keys 0 .. count - 1 are the visible ones
        share = (torch.ones((), dtype=torch.float32) / _denominators(case, b).to(torch.float32)).to(case.dtype)
        out.append(torch.where(hit, share[:, :, None], torch.zeros((), dtype=case.dtype)))
    if case.kind == "prefill":
        out.append(torch.zeros(case.pad_tokens, case.heads, case.vd, dtype=case.dtype))
    return out


def expected_selector(case, inputs):
    """Per sequence ``[rows, H, vd]`` fp64: the softmax (sink term in the denominator) of the exact scores over the visible keys,
    times the probes."""
    family, span = inputs.family, case.span(inputs.family)
    w = weights(case, family)
    j = probe_index(case, family)
    out = []
    for b, n in enumerate(case.kv_lens):
        rows, valid = case.rows(b), case.valid_len(b)
        if n == 0:
            out.append(torch.zeros(rows, case.heads, case.vd, dtype=torch.float64))
            continue
        q = inputs.q64[b]
        s = torch.einsum("ihd,sd->ihs", q[..., case.nope:], _dense_kpe(case, b, family)[:valid])
        if family == SEL_NOPE:
            lat = _dense_latent(case, b, family, inputs.base)[:valid]
            q_abs = torch.einsum("ihd,hdr->ihr", q[..., :case.nope], w[:, :case.nope])
            s = s + torch.einsum("ihr,sr->ihs", q_abs, lat)
        mask = (torch.arange(valid)[None, :] < case.counts(b)[:, None])[:, None, :]
        s = torch.where(mask, s, float("-inf"))
        sink = torch.full((rows, case.heads, 1), float("-inf"), dtype=torch.float64)
        if case.sink:
            sink = sink_logits(case).to(torch.float64)[None, :, None].expand(rows, -1, -1)
        p = torch.softmax(torch.cat([s, sink], dim=-1), dim=-1)[..., :-1]
        p = torch.where(mask.any(dim=-1, keepdim=True), p, torch.zeros((), dtype=torch.float64))      # rows that see no key
        o_lat = torch.zeros(rows, case.heads, span, dtype=torch.float64)
        o_lat.index_add_(2, (torch.arange(valid) - inputs.base) % span, p)
        out.append(torch.gather(o_lat, 2, j[None].expand(rows, -1, -1)))
    if case.kind == "prefill":
        out.append(torch.zeros(case.pad_tokens, case.heads, case.vd, dtype=torch.float64))
    return out


# ---- the comparer -----------------------------------------------------------------------------------------------------
def compare(case, inputs, got, want, limit=None):
    """``(failures, worst)``: per failing element ``(sequence, row, head, probed key position, got, want)`` (sequence
    ``len(kv_lens)``: the padding rows; at most ``limit`` per sequence), and the worst deviation — in ulp of the storage type
    (map) or absolute (selectors).  The rule of `visibility.compare`: a map ``want`` of 0 must read exactly 0, any other within
    1 ulp; a selector within `SELECTOR_TOL`."""
    failures, worst = [], 0.0
    span, j = case.span(inputs.family), probe_index(case, inputs.family)
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
            pos = inputs.base + int(j[head, c])
            if inputs.family != MAP and b < len(case.kv_lens):                      # the position this channel stands for
                t = int(inputs.targets[b][row, head])
                pos = t if (t - inputs.base) % span == int(j[head, c]) else pos
            failures.append((b, row, head, pos, float(g[row, head, c]), float(w[row, head, c])))
    return failures, worst


def run_family(case, family, op, device="cpu", strides=(), extra=(), repeat=False, **call_kw):
    """Every launch of one family through ``op``; returns ``(failures, worst)`` over all of them.  ``strides`` / ``extra``: see
    `selector_plan`.  ``repeat``: each call is made twice and must return the same bits."""
    failures, worst = [], 0.0
    if family == MAP:
        plan = [(base, None) for base in bases(case)]
        inputs = Inputs(case, MAP)
    else:
        plan = selector_plan(case, family, strides, extra)
        inputs = Inputs(case, family, targets=plan[0][1])
    for base, targets in plan:
        if base != inputs.base:
            inputs.set_base(base)
        if targets is not None:
            inputs.set_targets(targets)
        got = inputs.call(op, device, **call_kw)
        if repeat:
            again = inputs.call(op, device, **call_kw)
            assert torch.equal(again.view(torch.int16), got.view(torch.int16)), "two calls, two results"
        want = expected_map(case, base) if family == MAP else expected_selector(case, inputs)
        f, w = compare(case, inputs, got, want, limit=FAILURES_LISTED)
        failures += f
        worst = max(worst, w)
    return failures, worst
