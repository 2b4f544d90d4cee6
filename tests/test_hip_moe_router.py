"""The MoE router's expert choice on every route, instance and tie (the rule and the tables: tests/router_pin.py).

Exact cases: logits that are exact in fp32 in any summation order, a quarter of the expert columns copies of another — every
slot of every token must equal `router_pin.expected_choice` (descending logit, ties -> lowest expert id) and every launch must
report the full tag of the instance the table names.  Random cases: every token well formed, every token that differs from
the fp64 choice excused under a margin taken from the reference's arithmetic, at most 0.1 % of the tokens differing."""
import pytest
import torch

import router_pin as R
from hip_utils import DEV, hip_cls, last_launch, to_cpu

pytestmark = pytest.mark.gpu


def _route(case, switch, monkeypatch):
    """(ids, gates, launch tag) of `mojo_hip_moe_gating` on `case`, MOJO_HIP_GATING = `switch` (None: by shape)."""
    op = hip_cls("MojoMoEGating")(hidden_size=case.hidden, num_experts=case.experts, top_k=case.k)
    with torch.no_grad():
        op.gate_weight.copy_(case.w)
    op = op.to(DEV)
    assert op.gate_weight.dtype == torch.float32
    if switch is None:
        monkeypatch.delenv("MOJO_HIP_GATING", raising=False)
    else:
        monkeypatch.setenv("MOJO_HIP_GATING", switch)
    idx, gates = to_cpu(op(case.x.to(DEV)))
    return idx, gates, last_launch()


def _id(v):
    return str(v).replace("torch.", "") if isinstance(v, torch.dtype) else None


@pytest.mark.parametrize("route,switch,experts,k,hidden,tokens,tag,dtype,dense", R.exact_case_list(), ids=_id)
def test_exact_choice_on_every_route_and_instance(route, switch, experts, k, hidden, tokens, tag, dtype, dense, monkeypatch):
    case = R.exact_router_case(experts, k, hidden, tokens, dtype, R.exact_seed(experts, k, hidden, tokens), dense)
    idx, gates, launched = _route(case, switch, monkeypatch)
    assert launched == tag, launched
    R.judge_exact(idx, gates, case)


@pytest.mark.parametrize("dtype", R.DTYPES_16, ids=_id)
@pytest.mark.parametrize("experts,k,hidden,tokens,tag", [(64, 8, 128, 600, "moe_gating:mfma:sk2"), (64, 8, 128, 100, "moe_gating:small:ep64:slices2"),
                                                            (64, 8, 100, 600, "moe_gating:general:tt1:ei1"), (8, 2, 512, 600, "moe_gating:e8")])
def test_default_routing_reaches_every_route(experts, k, hidden, tokens, tag, dtype, monkeypatch):
    """No switch: the shape alone picks the route, one shape per route, each with the exact answer."""
    case = R.exact_router_case(experts, k, hidden, tokens, dtype, 21, True)
    idx, gates, launched = _route(case, None, monkeypatch)
    assert launched == tag, launched
    R.judge_exact(idx, gates, case)


@pytest.mark.parametrize("dense", [True, False])
@pytest.mark.parametrize("dtype", R.DTYPES_16, ids=_id)
def test_routes_agree_slot_for_slot_on_one_exact_case(dtype, dense, monkeypatch):
    """One exact case with ties through every route its shape admits: the same ids, and — the routes sharing
    `gate_softmax_topk` over the same exact logits — the same gate bits.  This is what sends a token to the same experts in
    the decode step (few-token route) and in the prefill (matrix cores)."""
    case = R.exact_router_case(64, 8, 128, 600, dtype, 22, dense)
    got = {}
    for switch, tag in (("1", "moe_gating:general:tt1:ei1"), ("3", "moe_gating:small:ep64:slices2"), ("4", "moe_gating:mfma:sk2")):
        idx, gates, launched = _route(case, switch, monkeypatch)
        assert launched == tag, launched
        R.judge_exact(idx, gates, case)
        got[switch] = (idx, gates)
    for switch in ("3", "4"):
        assert torch.equal(got[switch][0], got["1"][0]) and torch.equal(got[switch][1], got["1"][1]), switch
    # E = 8: the eight-expert stream against the general and the few-token kernels.  Its softmax runs inside one lane (another
    # order of the eight additions), so its gates are held to the suite's bound, not to the bits.
    case = R.exact_router_case(8, 2, 512, 600, dtype, 23, dense)
    got = {}
    for switch, tag in (("1", "moe_gating:general:tt1:ei1"), ("2", "moe_gating:e8"), ("3", "moe_gating:small:ep16:slices2")):
        idx, gates, launched = _route(case, switch, monkeypatch)
        assert launched == tag, launched
        R.judge_exact(idx, gates, case)
        got[switch] = (idx, gates)
    assert torch.equal(got["2"][0], got["1"][0]) and torch.equal(got["3"][0], got["1"][0])
    assert torch.equal(got["3"][1], got["1"][1])
    torch.testing.assert_close(got["2"][1], got["1"][1], atol=R.GATE_ATOL, rtol=R.GATE_RTOL)


def _random_params():
    out = []
    for experts, k, hidden, tokens, dtype, std, seed, routes in R.random_case_list():
        for switch, tag in routes:
            name = f"{experts}-{k}-{hidden}-{tokens}-{_id(dtype)}-{std}-{switch or 'by_shape'}-{tag.split(':')[1]}"
            out.append(pytest.param(experts, k, hidden, tokens, dtype, std, seed, switch, tag, id=name))
    return out


@pytest.mark.parametrize("experts,k,hidden,tokens,dtype,std,seed,switch,tag", _random_params())
def test_random_choice_is_well_formed_and_excused(experts, k, hidden, tokens, dtype, std, seed, switch, tag, monkeypatch):
    """Continuous data on each route it reaches.  The margin is the reference's: delta_vec for the vector routes, delta_mfma
    (+ the split's stated 2^-16 |x o w_e|_2) for the matrix cores.  Device figures: DESIGN §4.21."""
    case = R.random_router_case(experts, k, hidden, tokens, dtype, std, seed)
    idx, gates, launched = _route(case, switch, monkeypatch)
    assert launched == tag, launched
    print(f"router_pin: {launched}")
    R.judge_random(idx, gates, case, case.delta_mfma if ":mfma:" in tag else case.delta_vec)
