"""The exact-answer inputs of tests/visibility_mla.py through the two torch goldens of the MLA pair (CPU).

This ties the DEFINITION the GPU test (tests/test_hip_visibility_mla.py) checks the kernels against — causal visibility cut at
the first hole, the integer count with the sink's one, the probes — to the reference's semantics: each golden must differ from
the visibility-map expectation in 0 elements (0 ulp, exact zeros) and sit inside the selector tolerance (4 ulp of the storage
type at 1.0) on both selector codings.  The last tests run the comparer against goldens that are deliberately wrong, each a thin
wrapper of the golden (a subclass would register itself as a backend), and require that it flags each one and names the key.

Prefill cases never carry holes: the prefill golden cannot run with one (it views the decompressed keys with ``kv_len`` rows)."""
import dataclasses
import math

import pytest
import torch

import oracle.torch_golden
import visibility_mla as M
from visibility_mla import Case

BF16, F16 = torch.bfloat16, torch.float16
DECODE, PREFILL = "MojoPagedDecodeMLA", "MojoPagedPrefillMLA"
GOLDENS = {DECODE: oracle.torch_golden.TorchPagedDecodeMLA, PREFILL: oracle.torch_golden.TorchPagedPrefillMLA}
# (nope, rope, vd, r, heads, page)
DIMS = [(64, 32, 64, 32, 8, 16), (128, 64, 128, 512, 8, 32), (96, 32, 128, 64, 16, 16), (128, 64, 128, 256, 4, 8)]
DECODE_LENS = (250, 77, 19, 1, 16, 0)
PREFILL_LENS = dict(kv_lens=(250, 77, 19, 0), q_lens=(100, 77, 3, 0), pad_tokens=2)


def dims_kw(d):
    return dict(nope=d[0], rope=d[1], vd=d[2], r=d[3], heads=d[4], page=d[5])


def cases():
    out = []
    for dtype in (BF16, F16):
        for di, d in enumerate(DIMS):
            for sink in (False, True):
                out.append(Case(DECODE, "decode", DECODE_LENS, dtype=dtype, sink=sink, seed=di, **dims_kw(d)))
                out.append(Case(PREFILL, "prefill", dtype=dtype, sink=sink, seed=di, **PREFILL_LENS, **dims_kw(d)))
            # holes (decode only): the golden drops the tail behind the first negative id, and the dropped keys do not count
            lens = (250, 77, 40, 70)
            holes = tuple((b, p) for b, p in ((0, 5), (1, 1), (2, 2), (3, 3), (3, 1)) if p * d[5] < lens[b])
            out.append(Case(DECODE, "decode", lens, holes=holes, dtype=dtype, sink=di % 2 == 0, seed=9, **dims_kw(d)))
        out.append(Case(DECODE, "decode", (1000, 513, 0, 3), dtype=dtype, seed=3, **dims_kw(DIMS[1])))
        out.append(Case(DECODE, "decode", (1500, 1025, 40), dtype=dtype, seed=4, code_bits=11, **dict(dims_kw(DIMS[0]), page=1)))
    return out


def case_id(c):
    return (f"{c.op[9:]}-{str(c.dtype)[6:]}-{c.heads}x{c.nope}+{c.rope}x{c.vd}-r{c.r}-p{c.page}{'-sink' if c.sink else ''}"
            f"{'-holes' if c.holes else ''}{f'-bits{c.code_bits}' if c.code_bits != 10 else ''}-n{max(c.kv_lens)}")


WORST = {}


@pytest.mark.parametrize("case", cases(), ids=case_id)
def test_goldens_return_the_definition(case):
    golden = case.make(GOLDENS[case.op])
    failures, ulp = M.run_family(case, M.MAP, golden)
    assert not failures and ulp == 0, M.report(failures)                      # 0 ulp, exact zeros
    for family in (M.SEL_ROPE, M.SEL_NOPE):
        failures, err = M.run_family(case, family, golden, strides=(32, 64) + ((case.page,) if case.page >= 16 else ()))
        assert not failures, family + "\n" + M.report(failures)
        WORST[case.op, family] = max(WORST.get((case.op, family), 0.0), err)
        print(f"{case_id(case)}: map 0 ulp, {family} max |err| {err:.3e}")


def test_every_golden_was_run():
    assert {c.op for c in cases()} == set(GOLDENS)
    for (op, family), err in sorted(WORST.items()):                               # (with -s: the figures DESIGN §4.17 quotes)
        print(f"{op} {family}: map 0 ulp, worst |err| {err:.3e}")


@pytest.mark.parametrize("case", [
    Case(DECODE, "decode", (1000, 129, 17, 0), holes=((0, 20),), **dims_kw(DIMS[1])),
    Case(DECODE, "decode", (300, 31), **dims_kw(DIMS[0])),
    Case(PREFILL, "prefill", (300, 63), (63, 63), **dims_kw(DIMS[2]))], ids=case_id)
@pytest.mark.parametrize("family", [M.SEL_ROPE, M.SEL_NOPE])
def test_selector_plan_meets_every_candidate(case, family):
    """Every row's own edges, and both sides of every stride edge and extra position the sequence sees, land under a head
    whose probes contain them."""
    strides, extra, span = (32, 64, case.page), (5, 6), case.span(family)
    j = M.probe_index(case, family)
    plan = M.selector_plan(case, family, strides, extra)
    for b, n in enumerate(case.kv_lens):
        landed = [set() for _ in range(case.rows(b))]
        for base, targets in plan:
            for i, h in ((i, h) for i in range(case.rows(b)) for h in range(case.heads)):
                t = int(targets[b][i, h])
                if (t - base) % span in set(j[h].tolist()):
                    landed[i].add(t)
        if n > 0:
            assert all(set(M.own_candidates(case, b, i)) <= landed[i] for i in range(case.rows(b)))
            edges = M.edge_candidates(case, b, strides, extra)
            assert set(edges) <= set().union(*landed)
            valid = case.valid_len(b)
            want = {t for m in range(1, n) if any(m % s == 0 for s in strides) for t in (m - 1, m)} | set(extra)
            assert set(edges) == {t for t in want if t < valid}
            if case.holes and b == 0:
                assert {valid - 1, valid} <= landed[0]


# ---- the comparer sees a wrong visible set and names the key -----------------------------------------------------------
# n <= 70 visible keys per row: bf16 resolves n +- 1 up to n = 127
D0 = dims_kw((64, 32, 64, 32, 4, 16))
WRONG_D = Case(DECODE, "decode", (40, 23, 70), seed=6, **D0)
WRONG_P = Case(PREFILL, "prefill", (40, 23), (20, 9), seed=6, **D0)
WRONG_H = Case(DECODE, "decode", (40, 23, 70), holes=((0, 1), (2, 3)), seed=6, **D0)
WRONG_S = dataclasses.replace(WRONG_D, sink=True)


def _flagged(case, golden, inputs=None):
    inputs = inputs or M.Inputs(case, M.MAP)
    failures = []
    for base in M.bases(case):                              # every key of every sequence is probed
        inputs.set_base(base)
        failures += M.compare(case, inputs, inputs.call(golden), M.expected_map(case, base))[0]
    leaked = {(b, r, p) for b, r, _, p, g, w in failures if w == 0}
    dropped = {(b, r, p) for b, r, _, p, g, w in failures if w != 0 and g == 0}
    doubled = {(b, r, p) for b, r, _, p, g, w in failures if w != 0 and g > w}
    return failures, leaked, dropped, doubled


def _rows(case):
    """(sequence, row, position) of every query row."""
    return [(b, i, n - case.rows(b) + i) for b, n in enumerate(case.kv_lens) for i in range(case.rows(b))]


@pytest.mark.parametrize("case", [WRONG_D, WRONG_P, WRONG_H, WRONG_S], ids=["decode", "prefill", "holes", "sink"])
def test_the_true_goldens_are_clean(case):
    assert not _flagged(case, case.make(GOLDENS[case.op]))[0]


class Wrong:
    """A golden made wrong on purpose: the golden itself behind another ``forward`` (its parameters show through)."""

    def __init__(self, case, forward=None, decompress=None):
        self.golden = case.make(GOLDENS[case.op])
        self.wrong = forward
        if decompress is not None:
            right = self.golden._decompress
            self.golden._decompress = lambda c_kv, k_pe: right(*decompress(c_kv, k_pe))

    def __getattr__(self, name):
        return getattr(self.golden, name)

    def forward(self, *args, **kw):
        return self.golden.forward(*args, **kw) if self.wrong is None else self.wrong(self.golden, *args, **kw)


def _steps(cu_lens, sign):
    """``cu`` of lengths that are each one longer (shorter) than those of ``cu_lens``."""
    return cu_lens + sign * torch.arange(cu_lens.numel(), dtype=torch.int32)


def _edge_short(golden, q, c, pe, cu_q, table, softmax_scale=None, cu_total_seq_lens=None):
    """Every row one position early: it misses its own key."""
    return golden.forward(q, c, pe, cu_q, table, softmax_scale, _steps(cu_total_seq_lens, -1))


def test_comparer_flags_a_causal_edge_one_short():
    _, leaked, dropped, _ = _flagged(WRONG_P, Wrong(WRONG_P, _edge_short))
    assert dropped == {(b, i, p) for b, i, p in _rows(WRONG_P)} and not leaked


def _decode_long(golden, q, c, pe, lens, table, softmax_scale=None):
    return golden.forward(q, c, pe, lens + 1, table, softmax_scale)


def _prefill_long(golden, q, c, pe, cu_q, table, softmax_scale=None, cu_total_seq_lens=None):
    return golden.forward(q, c, pe, cu_q, table, softmax_scale, _steps(cu_total_seq_lens, 1))


@pytest.mark.parametrize("case,wrong", [(WRONG_D, _decode_long), (WRONG_P, _prefill_long)], ids=["decode", "prefill"])
def test_comparer_flags_a_length_one_too_long(case, wrong):
    """``kv_len + 1``: every row moves one position on — key ``p + 1`` leaks — and the last row sees the slot behind the
    sequence's last key, whose poison takes the whole softmax: that slot's probe, which must read 0, reads 1."""
    failures, leaked, _, _ = _flagged(case, Wrong(case, wrong))
    rows = _rows(case)
    assert leaked >= {(b, i, p + 1) for b, i, p in rows}
    last = {(b, case.rows(b) - 1, n) for b, n in enumerate(case.kv_lens)}
    hits = [g for b, r, _, p, g, w in failures if (b, r, p) in last]
    assert len(hits) >= len(last) and all(g == 1.0 for g in hits)


TWICE = 2


def _key_twice(c_kv, k_pe):
    return torch.cat([c_kv, c_kv[TWICE:TWICE + 1]]), torch.cat([k_pe, k_pe[TWICE:TWICE + 1]])


def test_comparer_flags_a_key_counted_twice():
    failures, leaked, dropped, doubled = _flagged(WRONG_D, Wrong(WRONG_D, decompress=_key_twice))
    assert doubled == {(b, 0, TWICE) for b in range(3)} and not leaked and not dropped
    for b, r, _, p, g, w in failures:
        if p == TWICE:
            assert abs(g - 2.0 / (WRONG_D.kv_lens[b] + 1)) < 0.02 * g                # 2 / (n + 1)
    assert {b for b, *_ in failures} == {0, 1, 2}                                   # and the miscount shows on the other probes
    assert len(failures) > 3 * WRONG_D.heads


def _neighbour_latent(c_kv, k_pe):
    """``k_pe[t]`` paired with latent ``[t + 1]``."""
    return torch.roll(c_kv, -1, dims=0), k_pe


def test_selector_comparer_flags_a_latent_of_the_neighbouring_key():
    case = WRONG_D
    base, targets = M.selector_plan(case, M.SEL_ROPE, (16,))[0]
    inputs = M.Inputs(case, M.SEL_ROPE, base=base, targets=targets)
    want = M.expected_selector(case, inputs)
    assert not M.compare(case, inputs, inputs.call(Wrong(case)), want)[0]
    failures, _ = M.compare(case, inputs, inputs.call(Wrong(case, decompress=_neighbour_latent)), want)
    j = M.probe_index(case, M.SEL_ROPE)
    landed = {(b, 0, h, int(targets[b][0, h])) for b in range(3) for h in range(case.heads)
              if (int(targets[b][0, h]) - base) % case.r in set(j[h].tolist()) and int(targets[b][0, h]) < case.kv_lens[b] - 1}
    assert landed and {(b, r, h, p) for b, r, h, p, g, w in failures if w > 0.5} >= landed


def _table_filled(fill, tail=False):
    """Walks the hole (``tail``: and every page behind it) as ``fill`` names it."""
    def forward(golden, q, c, pe, lens, table, softmax_scale=None):
        gone = (table < 0).cumsum(dim=1) > 0 if tail else table < 0
        return golden.forward(q, c, pe, lens, torch.where(gone, fill, table), softmax_scale)
    return forward


def test_comparer_flags_a_hole_ignored():
    case, inputs = WRONG_H, M.Inputs(WRONG_H, M.MAP)
    _, leaked, dropped, _ = _flagged(case, Wrong(case, _table_filled(inputs.whole_table)), inputs)
    behind = {(b, 0, p) for b, n in enumerate(case.kv_lens) for p in range(case.valid_len(b), n)}
    assert behind and leaked == behind and not dropped
    assert {(0, 0, 16), (2, 0, 48)} <= leaked                                       # the first key behind each hole, by name


def test_comparer_flags_keys_behind_a_hole_counted_in_n():
    """The GQA pair's rule (keys behind the hole count, with zero K / V) is wrong here: nothing leaks, every probe reads
    ``1 / kv_len`` where ``1 / valid`` is due."""
    case, inputs = WRONG_H, M.Inputs(WRONG_H, M.MAP)
    zero = torch.full_like(inputs.whole_table, inputs.zero_page)
    failures, leaked, dropped, doubled = _flagged(case, Wrong(case, _table_filled(zero, tail=True)), inputs)
    assert not leaked and not dropped and not doubled
    assert {(b, p) for b, r, _, p, g, w in failures} == {(b, p) for b in (0, 2) for p in range(case.valid_len(b))}
    for b, r, _, p, g, w in failures:
        assert g == float(torch.tensor(1.0 / case.kv_lens[b]).to(case.dtype))


def _no_sink(golden, *args, **kw):
    sink = golden._parameters.pop("attn_sink")
    try:
        return golden.forward(*args, **kw)
    finally:
        golden._parameters["attn_sink"] = sink


def _sink_twice(golden, *args, **kw):
    once = golden.attn_sink.data
    golden.attn_sink.data = (once.float() + math.log(2.0)).to(once.dtype)            # exp(s) + exp(s)
    try:
        return golden.forward(*args, **kw)
    finally:
        golden.attn_sink.data = once


@pytest.mark.parametrize("wrong,extra", [(_no_sink, 0.0), (_sink_twice, 2.0)], ids=["left-out", "twice"])
def test_comparer_flags_a_wrong_sink(wrong, extra):
    """Even heads carry a sink logit of 0: their denominator is ``n + 1``; without the sink they read ``1 / n``, with two
    ``1 / (n + 2)``.  The odd heads (logit -30000) are right either way."""
    case = WRONG_S
    failures, leaked, dropped, _ = _flagged(case, Wrong(case, wrong))
    assert not leaked and not dropped
    assert {(b, p) for b, r, h, p, g, w in failures} == {(b, p) for b, n in enumerate(case.kv_lens) for p in range(n)}
    assert {h % 2 for b, r, h, p, g, w in failures} == {0}
    for b, r, h, p, g, w in failures:
        assert abs(g - 1.0 / (case.kv_lens[b] + extra)) <= 2.0 ** -8 * g
