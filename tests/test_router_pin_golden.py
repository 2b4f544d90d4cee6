"""The router rule of tests/router_pin.py against the torch oracle, on the host: every case the device test
runs is first shown to be one the reference itself passes, and the helpers are shown to reject planted faults."""
import pytest
import torch

import oracle  # noqa: F401
import router_pin as R
from oracle.torch_golden import TorchMoEGating


def _oracle(case):
    op = TorchMoEGating(hidden_size=case.hidden, num_experts=case.experts, top_k=case.k)
    with torch.no_grad():
        op.gate_weight.copy_(case.w)
    assert op.gate_weight.dtype == torch.float32
    idx, gates = op(case.x)
    return idx, gates.float()


def _id(v):
    return str(v).replace("torch.", "") if isinstance(v, torch.dtype) else None


@pytest.mark.parametrize("route,switch,experts,k,hidden,tokens,tag,dtype,dense", R.exact_case_list(), ids=_id)
def test_oracle_passes_the_exact_cases(route, switch, experts, k, hidden, tokens, tag, dtype, dense):
    case = R.exact_router_case(experts, k, hidden, tokens, dtype, R.exact_seed(experts, k, hidden, tokens), dense)
    idx, gates = _oracle(case)
    assert bool(R.well_formed(idx, gates, experts).all())
    delta_vec, delta_mfma, logits64 = R.deltas(case.x, case.w)
    assert delta_vec == 0.0 and torch.equal(logits64, case.logits64)            # the fp32 product is exact
    for delta in (delta_vec, delta_mfma):
        assert bool(R.excused(idx, gates, case.logits64, k, delta).all())
    free = R.tie_free(case.logits64, k)                                         # torch.topk leaves tie order open
    want_idx, want_gates = R.expected_choice(case.logits64, k)
    assert torch.equal(idx[free], want_idx[free])
    torch.testing.assert_close(gates.double(), want_gates, atol=R.GATE_ATOL, rtol=R.GATE_RTOL)   # equal logits, equal gates
    if tokens >= 64 and experts >= 16 and k < experts:                          # the copies do their work: ties inside and across k
        inside, across = R.tie_profile(case.logits64, k)
        assert bool(inside.any()) and bool(across.any()) and not bool(free.all())


def test_copy_pairs_cover_the_layouts():
    pairs = R.copy_pairs(384, 1)
    assert len(pairs) == 96 and len({e for p in pairs for e in p}) == 192
    assert (255, 256) in pairs                                                   # across the 256-column edge
    assert any(d - s >= 64 and (d - s) % 64 == 0 for s, d in pairs)              # same lane, another register slot
    assert any((d - s) % 64 != 0 for s, d in pairs)                              # different lanes
    assert any(s // 16 != d // 16 for s, d in pairs) and any(s // 256 != d // 256 for s, d in pairs)
    assert R.copy_pairs(1, 0) == [] and R.copy_pairs(2, 0) == []


@pytest.mark.parametrize("experts,k,hidden,tokens,dtype,std,seed,routes", R.random_case_list(), ids=_id)
def test_oracle_passes_the_random_cases(experts, k, hidden, tokens, dtype, std, seed, routes):
    case = R.random_router_case(experts, k, hidden, tokens, dtype, std, seed)
    idx, gates = _oracle(case)
    assert 0 < case.delta_vec < case.delta_mfma
    for delta in (case.delta_vec, case.delta_mfma):
        differ, _ = R.judge_random(idx, gates, case, delta)
        assert differ <= 0.0005 * tokens                                       # the reference alone: half the share a kernel gets


def _planted():
    exact = R.exact_router_case(100, 6, 128, 70, torch.bfloat16, 11, True)
    rand = R.random_router_case(64, 8, 1024, 256, torch.bfloat16, 0.02, 0)
    return exact, rand


def test_helpers_reject_planted_faults():
    exact, rand = _planted()
    idx, gates = R.expected_choice(rand.logits64, rand.k)
    gates = gates.float()
    assert bool(R.well_formed(idx, gates, rand.experts).all()) and bool(R.excused(idx, gates, rand.logits64, rand.k, 0.0).all())
    big = 1e9                                                                     # a margin that forgives every choice

    bad = idx.clone()                                                             # an id >= E
    bad[3, 2] = rand.experts
    assert R.well_formed(bad, gates, rand.experts).tolist() == [t != 3 for t in range(rand.tokens)]
    assert not bool(R.excused(bad, gates, rand.logits64, rand.k, big)[3])
    bad[3, 2] = -1
    assert not bool(R.well_formed(bad, gates, rand.experts)[3])

    bad = idx.clone()                                                             # a duplicate id
    bad[5, 7] = bad[5, 0]
    assert R.well_formed(bad, gates, rand.experts).tolist() == [t != 5 for t in range(rand.tokens)]

    for g in (float("nan"), 0.0, -0.25, 1.5):                                      # a gate outside (0, 1]
        badg = gates.clone()
        badg[9, 7] = g
        assert not bool(R.well_formed(idx, badg, rand.experts)[9])
    badg = gates.clone()                                                          # gates that rise along k
    badg[9, 6], badg[9, 7] = gates[9, 7], gates[9, 6]
    assert bool(gates[9, 6] > gates[9, 7]) and not bool(R.well_formed(idx, badg, rand.experts)[9])

    chosen = torch.gather(rand.logits64, 1, idx.long())                           # a swapped pair beyond delta
    t = int((chosen[:, 0] - chosen[:, 1]).argmax())
    assert float(chosen[t, 0] - chosen[t, 1]) > rand.delta_mfma
    bad, badg = idx.clone(), gates.clone()
    bad[t, 0], bad[t, 1] = idx[t, 1], idx[t, 0]
    badg[t, 0], badg[t, 1] = gates[t, 1], gates[t, 0]                              # (the gates follow their experts)
    ok = R.excused(bad, badg, rand.logits64, rand.k, rand.delta_mfma)
    assert ok.tolist() == [u != t for u in range(rand.tokens)]
    assert bool(R.excused(bad, badg, rand.logits64, rand.k, big)[t])              # it is the margin that refuses it

    order = torch.sort(-rand.logits64, dim=-1, stable=True).indices               # an expert beyond delta below the k-th place
    gap = torch.gather(rand.logits64, 1, order[:, rand.k - 1: rand.k + 1])
    t = int((gap[:, 0] - gap[:, 1]).argmax())
    bad = idx.clone()
    bad[t, rand.k - 1] = order[t, rand.k]
    badg = R.chosen_gates(rand.logits64, bad).float()
    assert bool(R.well_formed(bad, badg, rand.experts).all())
    assert not bool(R.excused(bad, badg, rand.logits64, rand.k, rand.delta_mfma)[t])

    bad = idx.clone()                                                             # a gate renormalised over the wrong set: the ids
    bad[t, rand.k - 1] = order[t, rand.k]                                         # move to the (k+1)-th expert, the gates do not
    assert bool(R.well_formed(bad, gates, rand.experts).all())
    assert not bool(R.excused(bad, gates, rand.logits64, rand.k, big)[t])
    assert bool(R.excused(bad, R.chosen_gates(rand.logits64, bad).float(), rand.logits64, rand.k, big)[t])
    p = torch.softmax(rand.logits64, -1)                                          # ... and one renormalised over k + 1 experts
    badg = (torch.gather(p, 1, idx.long()) / torch.gather(p, 1, order[:, : rand.k + 1]).sum(-1, keepdim=True)).float()
    assert not bool(R.excused(idx, badg, rand.logits64, rand.k, big).any())
    with pytest.raises(AssertionError):
        R.judge_random(idx, badg, rand, rand.delta_vec)

    # a tie broken toward the higher id: still a valid top-k set, so only `expected_choice` tells
    idx, gates = R.expected_choice(exact.logits64, exact.k)
    gates = gates.float()
    R.judge_exact(idx, gates, exact)
    _, across = R.tie_profile(exact.logits64, exact.k)
    t = int(across.nonzero()[0])
    order = torch.sort(-exact.logits64, dim=-1, stable=True).indices
    assert int(order[t, exact.k]) > int(idx[t, exact.k - 1])
    bad = idx.clone()
    bad[t, exact.k - 1] = order[t, exact.k]
    assert bool(R.excused(bad, gates, exact.logits64, exact.k, 0.0).all()) and bool(R.well_formed(bad, gates, exact.experts).all())
    assert R.differing(bad, exact.logits64, exact.k).tolist() == [u == t for u in range(exact.tokens)]
    with pytest.raises(AssertionError):
        R.judge_exact(bad, gates, exact)
    inside, _ = R.tie_profile(exact.logits64, exact.k)                            # ... and a tie inside the first k, swapped
    t = int(inside.nonzero()[0])
    chosen = torch.gather(exact.logits64, 1, idx.long())
    j = int((chosen[t, :-1] == chosen[t, 1:]).nonzero()[0])
    bad = idx.clone()
    bad[t, j], bad[t, j + 1] = idx[t, j + 1], idx[t, j]
    with pytest.raises(AssertionError):
        R.judge_exact(bad, gates, exact)
    with pytest.raises(AssertionError):                                           # the dtypes are part of the result
        R.well_formed(idx.long(), gates, exact.experts)
