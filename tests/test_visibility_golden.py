"""The exact-answer inputs of tests/visibility.py through all ten torch goldens of the paged attention family (CPU).

This ties the DEFINITION the GPU test (tests/test_hip_visibility.py) checks the kernels against — `visibility.visible`, the
integer count, the probes — to the reference's semantics: every golden must differ from the visibility-map expectation in 0
elements (0 ulp, exact zeros) and sit inside the selector tolerance (4 ulp of the storage type at 1.0).  The last test runs the
comparer against goldens with a deliberately wrong visible set and requires that it flags each one and names the key.

Rows of the n-step goldens with ``0 < len < S`` are left out: the goldens return NaN there (the hip classes store zeros, which
the GPU test checks against the definition)."""
import dataclasses

import pytest
import torch

import nstep_golden
import nstep_kv_int8_golden
import oracle.kv_int8
import oracle.kv_int8_swa
import oracle.swa
import oracle.torch_golden
import visibility as V
from visibility import Case

BF16, F16 = torch.bfloat16, torch.float16
GOLDENS = {
    "MojoPagedDecodeGQA": oracle.torch_golden.TorchPagedDecodeGQA,
    "MojoPagedPrefillGQA": oracle.torch_golden.TorchPagedPrefillGQA,
    "MojoPagedDecodeSWA": oracle.swa.TorchPagedDecodeSWA,
    "MojoPagedPrefillSWA": oracle.swa.TorchPagedPrefillSWA,
    "MojoPagedDecodeGQAWithKVDequant": oracle.kv_int8.TorchPagedDecodeGQAWithKVDequant,
    "MojoPagedPrefillGQAWithKVDequant": oracle.kv_int8.TorchPagedPrefillGQAWithKVDequant,
    "MojoPagedDecodeSWAWithKVDequant": oracle.kv_int8_swa.TorchPagedDecodeSWAWithKVDequant,
    "MojoPagedPrefillSWAWithKVDequant": oracle.kv_int8_swa.TorchPagedPrefillSWAWithKVDequant,
    "MojoPagedDecodeNstepSWA": nstep_golden.TorchPagedDecodeNstepSWA,
    "MojoPagedDecodeNstepSWAWithKVDequant": nstep_kv_int8_golden.TorchPagedDecodeNstepSWAWithKVDequant,
}
WINDOWS = [(None, None), (4, 15), (None, 64), (3, 0), (17, 1), (40, 30)]     # (glob, local); the last pair overlaps
DECODE_LENS = (250, 77, 19, 1, 16, 0)
PREFILL = dict(kv_lens=(250, 77, 19, 0), q_lens=(100, 77, 3, 0), pad_tokens=2)


def cases():
    out = []
    for dtype in (BF16, F16):
        for op in ("MojoPagedDecodeGQA", "MojoPagedDecodeGQAWithKVDequant"):
            out.append(Case(op, "decode", DECODE_LENS, dtype=dtype))
            out.append(Case(op, "decode", (130, 33), hq=4, hkv=4, d=64, page=32, layout="ABAB", dtype=dtype, seed=1))
        for op in ("MojoPagedPrefillGQA", "MojoPagedPrefillGQAWithKVDequant"):
            out.append(Case(op, "prefill", dtype=dtype, **PREFILL))
            out.append(Case(op, "prefill", (70, 33), (70, 1), hq=4, hkv=1, d=64, page=32, layout="ABAB", dtype=dtype, seed=1))
        # holes (the GQA pair): the gather stops at the first negative id; keys behind it count, with zero K and V
        out.append(Case("MojoPagedDecodeGQA", "decode", (250, 77, 40), holes=((0, 9), (1, 1)), dtype=dtype, seed=2))
        out.append(Case("MojoPagedPrefillGQA", "prefill", (250, 77), (100, 77), holes=((0, 9), (1, 2)), dtype=dtype, seed=2))
        for glob, local in WINDOWS:
            for op in ("MojoPagedDecodeSWA", "MojoPagedDecodeSWAWithKVDequant"):
                out.append(Case(op, "decode", DECODE_LENS, glob=glob, local=local, dtype=dtype, seed=3))
            for op in ("MojoPagedPrefillSWA", "MojoPagedPrefillSWAWithKVDequant"):
                out.append(Case(op, "prefill", glob=glob, local=local, dtype=dtype, seed=3, **PREFILL))
            for op in ("MojoPagedDecodeNstepSWA", "MojoPagedDecodeNstepSWAWithKVDequant"):
                out.append(Case(op, "nstep", (250, 77, 19, 4, 0), steps=4, glob=glob, local=local, dtype=dtype, seed=4))
                out.append(Case(op, "nstep", (66, 3), steps=3, hq=8, hkv=1, d=64, layout="ABAB", glob=glob, local=local,
                                dtype=dtype, seed=5))
    return out


def case_id(c):
    win = "" if c.op not in V.WINDOW_OPS else f"-g{c.glob}-l{c.local}"
    return f"{c.op[4:]}-{str(c.dtype)[6:]}-{c.hq}x{c.hkv}x{c.d}-p{c.page}{win}{'-holes' if c.holes else ''}"


WORST = {}


@pytest.mark.parametrize("case", cases(), ids=case_id)
def test_goldens_return_the_definition(case):
    golden = case.make(GOLDENS[case.op])
    failures, ulp = V.run_family(case, V.MAP, golden)
    assert not failures and ulp == 0, V.report(failures)                      # 0 ulp, exact zeros
    failures, err = V.run_family(case, V.SELECTOR, golden, strides=(16, case.page))
    assert not failures, V.report(failures)
    WORST[case.op] = max(WORST.get(case.op, 0.0), err)
    print(f"{case_id(case)}: map 0 ulp, selector max |err| {err:.3e}")


def test_every_golden_was_run():
    assert {c.op for c in cases()} == set(GOLDENS)
    for op, err in sorted(WORST.items()):                                         # (with -s: the figures DESIGN §4.17 quotes)
        print(f"{op}: map 0 ulp, selector worst |err| {err:.3e}")


@pytest.mark.parametrize("case", [
    Case("MojoPagedDecodeGQA", "decode", (1000, 129, 17, 0), hq=4, hkv=2, d=128, page=48),
    Case("MojoPagedPrefillSWA", "prefill", (300, 63), (63, 63), hq=4, hkv=2, d=128, page=32, glob=4, local=63),
    Case("MojoPagedDecodeNstepSWA", "nstep", (1000, 2), steps=4, hq=8, hkv=1, d=64)], ids=case_id)
def test_selector_plan_meets_every_candidate(case):
    """Every row's own edges, and both sides of every tile and page edge a row sees, under a head whose kv head probes them."""
    strides, span = (16, case.page), case.hkv * case.d
    for b, n in enumerate(case.kv_lens):
        landed = [set() for _ in range(case.rows(b))]
        for base, targets in V.selector_plan(case, strides):
            for i, h in ((i, h) for i in range(case.rows(b)) for h in range(case.hq)):
                if (int(targets[b][i, h]) - base) % span // case.d == case.kv_head(h):
                    landed[i].add(int(targets[b][i, h]))
        if n > 0:
            assert all(set(V._own_candidates(case, b, i)) <= landed[i] for i in range(case.rows(b)))
            edges = V._edge_candidates(case, b, strides)
            assert set(edges) <= set().union(*landed)
            if case.local is None and case.glob is None and n >= case.rows(b):
                assert set(edges) == {t for m in range(1, n) if m % 16 == 0 or m % case.page == 0 for t in (m - 1, m)}


# ---- the comparer sees a wrong visible set and names the key -----------------------------------------------------------
# n <= 10 visible keys per row (bf16 resolves n +- 1 up to n = 127), no page inside the window gap
WRONG = Case("MojoPagedPrefillSWA", "prefill", (40, 23), (20, 9), hq=4, hkv=2, d=64, page=16, glob=4, local=5, seed=6)


def _flagged(case, golden, inputs=None):
    inputs = inputs or V.Inputs(case, V.MAP)
    got = inputs.call(golden)
    failures, _ = V.compare(case, inputs, got, V.expected_map(case, inputs.base))
    leaked = {(b, r, p) for b, r, _, p, g, w in failures if w == 0}
    dropped = {(b, r, p) for b, r, _, p, g, w in failures if w != 0 and g == 0}
    doubled = {(b, r, p) for b, r, _, p, g, w in failures if w != 0 and g > w}
    return failures, leaked, dropped, doubled


def _rows(case):
    """(sequence, row, position) of every query row."""
    return [(b, i, n - case.q_lens[b] + i) for b, n in enumerate(case.kv_lens) for i in range(case.q_lens[b])]


def test_the_true_mask_is_clean():
    assert not _flagged(WRONG, WRONG.make(GOLDENS[WRONG.op]))[0]


@pytest.mark.parametrize("what", ["local+1", "local-1", "glob-1"])
def test_comparer_flags_a_wrong_window(what):
    kw = {"local+1": dict(local=6), "local-1": dict(local=4), "glob-1": dict(glob=3)}[what]
    golden = dataclasses.replace(WRONG, **kw).make(GOLDENS[WRONG.op])         # the golden of ANOTHER window on WRONG's inputs
    failures, leaked, dropped, doubled = _flagged(WRONG, golden)
    rows = _rows(WRONG)
    if what == "local+1":                                  # the key one below the window's lower edge leaks
        assert leaked == {(b, i, p - 6) for b, i, p in rows} and not dropped
    elif what == "local-1":                                # the window's lowest key is dropped
        assert dropped == {(b, i, p - 5) for b, i, p in rows} and not leaked
    else:                                                  # the last global key is dropped
        assert dropped == {(b, i, 3) for b, i, p in rows} and not leaked
    # and the miscount shows on every other probe of every row (n <= 10: 1 / n and 1 / (n +- 1) are many ulp apart)
    assert {(b, i) for b, i, *_ in failures} == {(b, i) for b, i, _ in rows}
    assert len(failures) >= 5 * len(rows) * WRONG.group


def test_comparer_flags_a_causal_edge_one_short(monkeypatch):
    def short(q_len, kv_len, local, glob):
        mask = V.window_mask(q_len, kv_len, local, glob)
        pos = torch.arange(q_len)[:, None] + (kv_len - q_len)
        return mask & (torch.arange(kv_len)[None, :] < pos)
    monkeypatch.setattr(oracle.swa, "window_mask", short)
    _, leaked, dropped, _ = _flagged(WRONG, WRONG.make(GOLDENS[WRONG.op]))
    assert dropped == {(b, i, p) for b, i, p in _rows(WRONG)} and not leaked


def test_comparer_flags_a_length_one_too_long():
    """``kv_len + 1``: every row moves one position on — key ``p + 1`` leaks — and the last row sees the slot behind the
    sequence's last key, whose poison takes the whole softmax: that slot's probe, which must read 0, reads 1."""
    inputs = V.Inputs(WRONG, V.MAP)
    inputs.cu_kv = V.cu([n + 1 for n in WRONG.kv_lens])
    failures, leaked, _, _ = _flagged(WRONG, WRONG.make(GOLDENS[WRONG.op]), inputs)
    assert leaked >= {(b, i, p + 1) for b, i, p in _rows(WRONG)}
    last = {(b, WRONG.q_lens[b] - 1, n) for b, n in enumerate(WRONG.kv_lens)}
    assert all(g == 1.0 for b, r, _, p, g, w in failures if (b, r, p) in last)


def test_comparer_flags_a_key_counted_twice(monkeypatch):
    twice = 2                                               # a global key: every row sees it

    def pages(cache, table_row, kv_len):
        x = oracle.paged.index_pages(cache, table_row, kv_len)
        return torch.cat([x, x[:, twice:twice + 1]], dim=1)

    def mask(q_len, kv_len, local, glob):
        m = V.window_mask(q_len, kv_len, local, glob)
        return torch.cat([m, m[:, twice:twice + 1]], dim=1)
    monkeypatch.setattr(oracle.swa, "index_pages", pages)
    monkeypatch.setattr(oracle.swa, "window_mask", mask)
    failures, leaked, dropped, doubled = _flagged(WRONG, WRONG.make(GOLDENS[WRONG.op]))
    assert doubled == {(b, i, twice) for b, i, _ in _rows(WRONG)} and not leaked and not dropped
    assert all(abs(g / w - 2 * (1 / w) / (1 / w + 1)) < 0.02 for b, r, _, p, g, w in failures if p == twice)   # 2 / (n + 1)


def test_selector_comparer_flags_a_value_of_the_neighbouring_key(monkeypatch):
    """K[t] paired with V[t + 1]: the selector reads its 1.0 on the neighbouring channel."""
    case = Case("MojoPagedDecodeSWA", "decode", (40, 23), hq=4, hkv=2, d=64, seed=7)
    base, targets = V.selector_plan(case, (16,))[0]
    inputs = V.Inputs(case, V.SELECTOR, base=base, targets=targets)
    golden, want = case.make(GOLDENS[case.op]), V.expected_selector(case, inputs)
    assert not V.compare(case, inputs, inputs.call(golden), want)[0]

    def pages(cache, table_row, kv_len):
        x = oracle.paged.index_pages(cache, table_row, kv_len)
        return torch.roll(x, -1, dims=1) if cache is inputs.v else x
    monkeypatch.setattr(oracle.swa, "index_pages", pages)
    failures, _ = V.compare(case, inputs, inputs.call(golden), want)
    span = case.hkv * case.d
    landed = {(b, 0, h, int(targets[b][0, h])) for b in range(2) for h in range(case.hq)
              if (int(targets[b][0, h]) - base) % span // case.d == case.kv_head(h) and int(targets[b][0, h]) < case.kv_lens[b] - 1}
    assert landed and {(b, r, h, p) for b, r, h, p, g, w in failures if w > 0.5} >= landed
