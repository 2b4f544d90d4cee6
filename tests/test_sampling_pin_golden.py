"""The sampling pin of tests/sampling_pin.py on the host: the rule against the torch golden on every case, no
undecidable row, the geometry mirror against the library's workspace query, every case against what its note claims, the
search depths the case list reaches per dtype and pass, and the judge against four planted wrong answers."""
import numpy as np
import pytest
import torch

import oracle.sampling as G
import sampling_pin as P
from mojo_opset_amd.backends.hip.operators import sampling as S

NAMES = list(P.CASES)


@pytest.mark.parametrize("name", NAMES)
def test_rule_equals_the_golden_and_no_row_is_undecidable(name):
    c, judged = P.get_case(name), P.judged_of(name)
    values, indices = G.topk_sorted(c.logits.float(), c.k)
    assert torch.equal(indices, c.indices) and torch.equal(values, c.values)
    assert torch.equal(judged.indices, c.indices) and torch.equal(judged.values, c.values)
    assert not bool(torch.isnan(judged.probs32).any()) and bool(torch.isfinite(c.values[:, 0]).all())
    print(f"{name}: top_p {c.top_p} delta {judged.delta:.3e} nearest approach {judged.nearest:.3e} kept {judged.kept.tolist()}")
    assert int(judged.undecidable.sum()) == 0 and judged.nearest > 4 * judged.delta
    if c.family == "constant":
        assert indices.tolist() == [list(range(c.k))] * c.rows
    P.judge_filter(name, judged.probs32.to(c.dtype), judged.indices, name)      # the golden passes its own judge


def test_top_p_on_a_constant_row_sits_between_the_grid_points():
    row = torch.full((1, 4000), 1.5)
    values, _ = P.expected_topk(row, 100)
    assert P.choose_top_p(values) == 0.7005
    from sampling_judge import Judged

    assert Judged(row, 0.7005, 1, 100, P.NEG_INF).kept.tolist() == [71]
    assert bool(Judged(row, 0.7, 1, 100, P.NEG_INF).undecidable.all())           # a grid value is undecidable


@pytest.mark.parametrize("name", NAMES)
def test_mirror_matches_the_library_workspace_bytes(name):
    c = P.get_case(name)
    for slices in P.SLICES:
        geo = P.geometry(c.rows, c.vocab, c.k, slices)
        assert geo.bytes == S.workspace_bytes(c.rows, c.vocab, c.k, slices), (name, slices, geo.tag)
        assert geo.segments[0][0] == 0 and max(e for _, e in geo.segments) == c.vocab
        assert all(a == b for (_, a), (b, _) in zip(geo.segments, geo.segments[1:]) if b < c.vocab)


def test_mirror_gives_the_recorded_geometries():
    assert [P.geometry(20, 151936, 1000, s).tag for s in (0, 1, 2, 8)] == ["slices13x1", "slices1x10", "slices2x5", "slices8x2"]
    assert [P.geometry(1, 1049216, 300, s).tag for s in (0, 1)] == ["slices253x1", "slices1x65"]
    geo = P.geometry(1, 40000, 64, 4096)
    assert (geo.slices, geo.sub, geo.seg_len, geo.kcap) == (625, 1, 64, 64)
    geo = P.geometry(1, 65, 65, 2)                                              # two slices, the second with one key
    assert geo.segments == ((0, 64), (64, 65))
    assert any(e - s < 1024 for s, e in P.geometry(2, 40000, 1024, 4096).segments)   # a segment shorter than K
    vocab = P.straddling_vocab(300, 1)
    for s in (0, 1):
        assert any(a + 1536 <= (1 << 20) <= b - 1536 for a, b in P.geometry(1, vocab, 300, s).segments)


def _tie_group(c, row):
    x = c.logits[row].float()
    return torch.nonzero(x == c.values[row, c.k - 1]).flatten().numpy()


@pytest.mark.parametrize("name", NAMES)
def test_every_case_does_what_its_note_claims(name):
    c = P.get_case(name)
    assert c.note["text"] and c.family in name
    for slices, kind, row, want in c.note["claims"]:
        geo = P.geometry(c.rows, c.vocab, c.k, slices)
        comps = P.composites_of(c.logits[row])
        what = (name, slices, kind, row, want)
        if kind == "straddle":
            nxt = P.expected_topk(c.logits[row:row + 1].float(), c.k + 1)[0][0] if c.k < c.vocab else None
            assert (nxt is not None and bool(nxt[c.k - 1] == nxt[c.k])) == want, what
        elif kind == "span":
            members = _tie_group(c, row)
            assert sum(bool(((members >= s) & (members < e)).any()) for s, e in geo.segments) >= want, what
        elif kind in ("a", "a_bin4"):
            segs = [(s, e) for s, e in geo.segments if e > s]
            if kind == "a":
                hits = [(s, e) for s, e in segs if P.cut_depth(comps[s:e], min(c.k, e - s)) == want]
                assert hits, what
                assert P.search_depth(comps[hits[0][0]:hits[0][1]], min(c.k, hits[0][1] - hits[0][0])) == want, what
            else:
                s, e = next((s, e) for s, e in segs if s <= (1 << 20) < e)
                assert P.search_walk(comps[s:e], min(c.k, e - s))[3][0] == want, what
        else:
            walk = P.search_walk(np.concatenate(P.candidates_of(comps, geo, c.k)), c.k)
            assert (len(walk) if kind == "b" else walk[3][0]) == want, (what, walk)


def test_the_case_list_reaches_every_search_depth():
    """Per dtype: the depths that pass A (some segment) and pass B reach over every case and slice count are exactly
    `P.REACHABLE` (sampling_pin's docstring says why bf16 / fp16 cannot end in the third key digit, and why only the rows of
    more than 2^20 columns end in the first index digit)."""
    seen = {d: (set(), set()) for d in P.DTYPES}
    checked = 0
    for name in NAMES:
        c = P.get_case(name)
        for slices in P.SLICES:
            geo = P.geometry(c.rows, c.vocab, c.k, slices)
            for row in range(c.rows):
                a, b = P.depths(c.logits[row], geo, c.k)
                seen[c.dtype][0].update(a)
                seen[c.dtype][1].add(b)
                if slices == 1 and c.vocab <= 40000 and row == 0:               # the closed form against the digit walk itself
                    assert (a, b) == P.depths(c.logits[row], geo, c.k, walk=P.search_depth), name
                    checked += 1
    for dtype, (a, b) in seen.items():
        print(f"{P.SHORT[dtype]}: pass A reaches {sorted(a)}, pass B reaches {sorted(b)}")
        assert a == P.REACHABLE[dtype] and b == P.REACHABLE[dtype], (dtype, sorted(a), sorted(b))
    assert checked >= 60


def _wrong_answers(name):
    """(what, indices) of the four planted answers, for the rows of one case."""
    c = P.get_case(name)
    x = c.logits.double().numpy() + 0.0
    col = np.arange(c.vocab)
    higher = np.stack([np.lexsort((-col, -row))[:c.k] for row in x])
    yield "ties broken by the higher index", torch.from_numpy(higher).long()
    yield "torch.topk's own order", torch.topk(c.logits.float(), c.k).indices
    if c.k < c.vocab:
        swapped = c.indices.clone()
        swapped[:, c.k - 1] = P.expected_topk(c.logits.float(), c.k + 1)[1][:, c.k]
        yield "the two candidates around position K swapped", swapped
    yield "the right set ordered by index", torch.sort(c.indices, dim=-1).values


@pytest.mark.parametrize("name", ["two_level-k64-fp32", "two_level-k1024-bf16", "constant-k64-fp16", "edges-k1023-fp32",
                                  "key_digits-d2x3-bf16", "minus_inf-fp32"])
def test_judge_rejects_the_planted_wrong_answers(name):
    c, judged = P.get_case(name), P.judged_of(name)
    probs = judged.probs32.to(c.dtype)
    P.judge_filter(name, probs, judged.indices.clone(), name)
    rejected = []
    for what, indices in _wrong_answers(name):
        if torch.equal(indices, c.indices):                                     # (a constant row IS ordered by index)
            continue
        with pytest.raises(AssertionError):
            P.judge_filter(name, probs, indices, what)
        rejected.append(what)
    print(name, rejected)
    assert "ties broken by the higher index" in rejected and "the two candidates around position K swapped" in rejected
    assert name.startswith("constant") or len(rejected) == 4                    # (torch.topk's order included: it differs)
    bad = probs.clone()                                                         # a probability past the cut, and one off its value
    if c.filter_value == P.NEG_INF and int(judged.kept[0]) < c.k:
        bad[0, c.k - 1] = 1e-3
        with pytest.raises(AssertionError):
            P.judge_filter(name, bad, judged.indices, "a probability past the cut")
    bad = probs.clone()
    bad[0, 0] = bad[0, 0] * 1.02
    with pytest.raises(AssertionError):
        P.judge_filter(name, bad, judged.indices, "a probability 2 % off")


def test_torch_topk_order_differs_somewhere():
    """The second planted answer is a real one: on at least one tied case torch.topk's order is not the pinned one."""
    differs = [n for n in ("two_level-k64-fp32", "two_level-k1024-bf16", "edges-k1023-fp32")
               if not torch.equal(torch.topk(P.get_case(n).logits.float(), P.get_case(n).k).indices, P.get_case(n).indices)]
    assert differs
