"""`MojoGatedDeltaRule` / `MojoGatedDeltaRuleUpdateState` (`LINEAR_ATTN_OPS`): the core goldens and the chunk yardstick against the
fp64 model of tests/gated_delta_golden.py without a GPU, and `HIPGatedDeltaRule` / `HIPGatedDeltaRuleUpdateState`
(csrc/gated_delta_rule.hip) against the same model on one.

Prefill bound, per tensor: ``|got - model64| <= 2 E + u |model64|`` with ``E`` the largest error of `chunk_bf16_yardstick` on the
same case (computed here on the CPU), ``u = 2^-8`` for the bf16 output and 0 for the fp32 state.  Update bound (fp32 arithmetic,
derived): output ``u |out64| + 2 Dk 2^-24 scale |S64|^T |q^|``, state ``2 Dk 2^-24 sum_t |k^| (x) |d64| + 2^-23 sum_t |S64|``: a
sequential fp32 sum of Dk terms errs by at most Dk 2^-24 of the sum of magnitudes, and two such sums feed each quantity.
Largest ``max |err| / bound`` measured on an MI355X over every case of this file: prefill 0.64 (output) and 0.64 (state); update
0.97 (output: the one rounding, whose largest error IS ``u |out64|``) and 0.49 (state).  An all-fp32 update kernel measured 1.03
for the state, and the fp32 golden on the CPU 1.52: ``d`` is a difference of nearly equal numbers, so the kernel sums ``S^T k^`` in
fp64."""
import functools
import sys
import types

import pytest
import torch

import mojo_opset_amd as mo
from mojo_opset_amd.backends.hip import lib as L
from mojo_opset_amd.backends.hip.operators.linear_attention import HIPGatedDeltaRule, HIPGatedDeltaRuleUpdateState, dv_slice_plan
from gated_delta_golden import build, chunk_bf16_yardstick

gpu = pytest.mark.gpu
UNIT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
DIMS = [(64, 64), (128, 128), (128, 64)]
HEADS = [(2, 2), (1, 2)]
VARIANTS = {"norm-init": (True, True), "plain-zero": (False, False)}        # (use_qk_l2norm, initial_state)


class TorchGatedDeltaRule(mo.MojoGatedDeltaRule):
    """The core class's golden ``forward`` as the ``torch`` backend."""
    supported_platforms_list = ["rocm", "cpu"]


class TorchGatedDeltaRuleUpdateState(mo.MojoGatedDeltaRuleUpdateState):
    supported_platforms_list = ["rocm", "cpu"]


@functools.lru_cache(maxsize=None)
def yardstick_error(*key):
    """(E_out, E_state) of `chunk_bf16_yardstick` on ``build(*key)``."""
    c = build(*key)
    out, state = chunk_bf16_yardstick(c["q"], c["k"], c["v"], c["g"], c["beta"], c["state"], norm=c["norm"])
    return float((out - c["out64"]).abs().max()), float((state - c["state64"]).abs().max())


def batch(cases, device="cpu", names=("q", "k", "v", "g", "beta")):
    return [torch.stack([c[n] for c in cases]).to(device) for n in names]


def states(cases, device="cpu"):
    return None if cases[0]["state"] is None else torch.stack([c["state"] for c in cases]).to(device)


def within_bound(what, got, want, slack, unit=0.0):
    got = got.detach().cpu().double()
    assert not torch.isnan(got).any()
    ratio = float(((got - want).abs() / (slack + unit * want.abs())).max())
    print(f"{what}: max |err| / bound = {ratio:.3f}")
    assert ratio <= 1.0
    return ratio


def prefill_within_bound(out, state, c, key):
    e_out, e_state = yardstick_error(*key)
    within_bound("out", out, c["out64"], 2 * e_out, UNIT[torch.bfloat16])
    if state is not None:
        within_bound("state", state, c["state64"], 2 * e_state)


def update_within_bound(out, state, c, dk, dtype):
    rel = 2 * dk * 2.0 ** -24
    within_bound("out", out, c["out64"], rel * c["mag_o"] + 1e-30, UNIT[dtype])
    within_bound("state", state, c["state64"], rel * c["mag_kd"] + 2.0 ** -23 * c["mag_s"] + 1e-30)


@pytest.mark.parametrize("variant", VARIANTS)
def test_core_goldens_against_the_fp64_model(variant):
    norm, init = VARIANTS[variant]
    key = (70, 64, 128, 1, 2, norm, init)
    c = build(*key)
    q, k, v, g, beta = batch([c])
    out, final = TorchGatedDeltaRule(norm)(q, k, v, g, beta, initial_state=states([c]), output_final_state=True)
    within_bound("out", out[0], c["out64"], 1e-5 * c["out64"].abs().max(), UNIT[torch.bfloat16])
    within_bound("state", final[0], c["state64"], 1e-5 * c["state64"].abs().max())
    cu = torch.tensor([0, 0, 70], dtype=torch.int32)                     # packed: an empty sequence, then the same tokens
    st = None if not init else torch.cat([states([c]), states([c])])
    packed, final2 = TorchGatedDeltaRule(norm)(q, k, v, g, beta, initial_state=st, output_final_state=True, cu_seqlens=cu)
    assert torch.equal(packed, out) and torch.equal(final2[1], final[0])
    assert torch.equal(final2[0], st[0] if init else torch.zeros_like(final[0]))
    c8 = build(8, 64, 128, 1, 2, norm, True)
    state = states([c8])
    got = TorchGatedDeltaRuleUpdateState(norm)(*batch([c8]), state)
    update_within_bound(got[0], state[0], c8, 64, torch.bfloat16)


@pytest.mark.parametrize("key", [(130, 64, 64, 2, 2, True, True), (200, 128, 128, 1, 2, False, True)])
def test_yardstick_formulas_in_fp32_match_the_fp64_model(key):
    c = build(*key)
    out, state = chunk_bf16_yardstick(c["q"], c["k"], c["v"], c["g"], c["beta"], c["state"], norm=c["norm"], operand=torch.float32)
    within_bound("out", out, c["out64"], 1e-5 * c["out64"].abs().max())
    within_bound("state", state, c["state64"], 1e-5 * c["state64"].abs().max())


def test_sets_constructor_and_plugin():
    names = ("MojoGatedDeltaRule", "MojoGatedDeltaRuleUpdateState")
    assert mo.LINEAR_ATTN_OPS == mo.core.LINEAR_ATTN_OPS == mo.core.operators.LINEAR_ATTN_OPS == names
    assert not set(names) & set(mo.__all__)
    assert TorchGatedDeltaRule().use_qk_l2norm and TorchGatedDeltaRuleUpdateState().use_qk_l2norm
    assert "use_qk_l2norm=False" in repr(TorchGatedDeltaRule(False))
    from mojo_opset_amd import plugin

    ref = types.ModuleType("stand_in_linear_attention_reference")
    cores = {n: type(n, (mo.core.MojoOperator,), {"forward": lambda self, *a, **k: None}) for n in names}
    vars(ref).update(cores)
    sys.modules[ref.__name__] = ref
    try:
        made = plugin.rebase_hip_backend(ref, platforms=["rocm", "cpu"])
    finally:
        del sys.modules[ref.__name__]
    for name, hip in zip(names, (HIPGatedDeltaRule, HIPGatedDeltaRuleUpdateState)):
        assert issubclass(made[name], cores[name]) and made[name].forward is hip.forward


@pytest.mark.parametrize("name", ["Dk 96", "Hv % Hk", "fp16 prefill", "T 9 update", "bf16 state", "row stride"])
def test_refusals_come_before_any_device_work(name):
    """CPU tensors: a refusal that came behind the first device step would be the loader's `MojoHipError` instead."""
    tokens, dk, hk, hv = (9 if name == "T 9 update" else 4), (96 if name == "Dk 96" else 64), 2, (3 if name == "Hv % Hk" else 2)
    dtype = torch.float16 if name == "fp16 prefill" else torch.bfloat16
    q, k = torch.zeros(1, tokens, hk, dk + 4, dtype=dtype), torch.zeros(1, tokens, hk, dk, dtype=dtype)
    q = q[..., :dk] if name == "row stride" else q[..., :dk].contiguous()
    v, g = torch.zeros(1, tokens, hv, 64, dtype=dtype), torch.zeros(1, tokens, hv)
    state = torch.zeros(1, hv, dk, 64, dtype=torch.bfloat16 if name == "bf16 state" else torch.float32)
    if name != "T 9 update":
        with pytest.raises(NotImplementedError):
            HIPGatedDeltaRule()(q, k, v, g, g, initial_state=state)
    if name != "fp16 prefill":
        with pytest.raises(NotImplementedError):
            HIPGatedDeltaRuleUpdateState()(q, k, v, g, g, state)


def run_prefill(cases, norm, device="cuda", fused=False, **kw):
    q, k, v, g, beta = batch(cases, device)
    if fused:                                                # the three column slices of one [B, T, 2 Hk Dk + Hv Dv] buffer
        (b, t, hk, dk), (hv, dv) = q.shape, v.shape[2:]
        buf = torch.cat([q.flatten(2), k.flatten(2), v.flatten(2)], dim=2)
        q, k, v = (x.unflatten(2, (h, d)) for x, (h, d) in zip(buf.split([hk * dk, hk * dk, hv * dv], dim=2),
                                                               ((hk, dk), (hk, dk), (hv, dv))))
        assert not v.is_contiguous()
    return HIPGatedDeltaRule(norm)(q, k, v, g, beta, initial_state=states(cases, device), output_final_state=True, **kw)


@gpu
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("hk,hv", HEADS)
@pytest.mark.parametrize("dk,dv", DIMS)
@pytest.mark.parametrize("tokens", [1, 63, 64, 65, 130])
def test_prefill_against_the_fp64_model(tokens, dk, dv, hk, hv, variant, monkeypatch):
    norm, init = VARIANTS[variant]
    key = (tokens, dk, dv, hk, hv, norm, init)
    c = build(*key)
    monkeypatch.setenv("MOJO_BACKEND", "hip")
    assert type(mo.MojoGatedDeltaRule()) is HIPGatedDeltaRule and type(mo.MojoGatedDeltaRuleUpdateState()) is HIPGatedDeltaRuleUpdateState
    forced = {}
    for dv_slice in (32, 64):                                # every plan the host can choose
        out, state = forced[dv_slice] = run_prefill([c], norm, dv_slice=dv_slice)
        assert L.last_launch() == f"gated_delta_rule:chunk64:dk{dk}:dvs{dv_slice}:batched"
        prefill_within_bound(out[0], state[0], c, key)
        again = run_prefill([c], norm, dv_slice=dv_slice)
        assert torch.equal(again[0], out) and torch.equal(again[1], state), "two calls differ"
    planned = run_prefill([c], norm)
    taken = forced[dv_slice_plan(1, hv, dv)]
    assert torch.equal(planned[0], taken[0]) and torch.equal(planned[1], taken[1])


@gpu
@pytest.mark.parametrize("cu_dtype", [torch.int32, torch.int64])
def test_packed_sequences_and_fused_buffer_slices(cu_dtype):
    lengths, dims = [1, 0, 66, 64, 130], (128, 128, 1, 2, True, True)
    cases = [build(max(n, 1), *dims, torch.bfloat16, False, i) for i, n in enumerate(lengths)]
    q, k, v, g, beta = (torch.cat([c[n][:ln] for c, ln in zip(cases, lengths)])[None].cuda() for n in ("q", "k", "v", "g", "beta"))
    cu = torch.tensor([0] + lengths, dtype=cu_dtype).cumsum(0).to(cu_dtype).cuda()
    out, final = HIPGatedDeltaRule()(q, k, v, g, beta, initial_state=states(cases, "cuda"), output_final_state=True, cu_seqlens=cu)
    assert L.last_launch().endswith(":packed")
    start = 0
    for i, (c, n) in enumerate(zip(cases, lengths)):
        if n == 0:
            assert torch.equal(final[i].cpu(), c["state"])
        else:
            prefill_within_bound(out[0, start:start + n], final[i], c, (n, *dims, torch.bfloat16, False, i))
        start += n
    two = [build(65, 128, 64, 1, 2, True, True, torch.bfloat16, False, s) for s in (0, 1)]          # batched, q / k / v read in place
    out, final = run_prefill(two, True, fused=True)
    for i, c in enumerate(two):
        prefill_within_bound(out[i], final[i], c, (65, 128, 64, 1, 2, True, True, torch.bfloat16, False, i))


@gpu
def test_edge_rows_and_continuation():
    key = (130, 64, 64, 2, 2, True, True, torch.bfloat16, True)  # g = 0, g = -8 per token, beta = 0 and beta = 1 rows
    c = build(*key)
    out, state = run_prefill([c], True)
    prefill_within_bound(out[0], state[0], c, key)
    key = (130, 128, 128, 1, 2, True, True)                      # 65 + 65 with the state handed over: the single run's bound
    c = build(*key)
    q, k, v, g, beta = batch([c], "cuda")
    op, state, outs = HIPGatedDeltaRule(), states([c], "cuda"), []
    for part in (slice(0, 65), slice(65, 130)):
        o, state = op(q[:, part], k[:, part], v[:, part], g[:, part], beta[:, part], initial_state=state, output_final_state=True)
        outs.append(o)
    prefill_within_bound(torch.cat(outs, dim=1)[0], state[0], c, key)


@gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("hk,hv", HEADS)
@pytest.mark.parametrize("dk,dv", DIMS)
@pytest.mark.parametrize("tokens", [1, 2, 8])
def test_update_against_the_fp64_model(tokens, dk, dv, hk, hv, dtype):
    norm = hk == 2                                                # the norm on for one head layout, off for the other
    cases = [build(tokens, dk, dv, hk, hv, norm, True, dtype, False, s) for s in (0, 1)]
    q, k, v, g, beta = batch(cases, "cuda")
    if hk == 1:                                                   # strided: q / k / v as slices of wider buffers
        q, k, v = (torch.cat([x, x], dim=3)[..., :x.shape[3]] for x in (q, k, v))
    state = states(cases, "cuda")
    kept = state.data_ptr()
    out = HIPGatedDeltaRuleUpdateState(norm)(q, k, v, g, beta, state)
    assert L.last_launch() == f"gated_delta_rule_update:dk{dk}:t{tokens}" and state.data_ptr() == kept
    for i, c in enumerate(cases):
        update_within_bound(out[i], state[i], c, dk, dtype)
    again = states(cases, "cuda")
    assert torch.equal(HIPGatedDeltaRuleUpdateState(norm)(q, k, v, g, beta, again), out) and torch.equal(again, state)


@gpu
def test_prefill_then_decode_and_graph_replay():
    key = (65, 128, 128, 1, 2, True, True)
    c = build(*key)
    q, k, v, g, beta = batch([c], "cuda")
    out, state = HIPGatedDeltaRule()(q[:, :64], k[:, :64], v[:, :64], g[:, :64], beta[:, :64], initial_state=states([c], "cuda"),
                                     output_final_state=True)
    step = HIPGatedDeltaRuleUpdateState()
    last = step(q[:, 64:], k[:, 64:], v[:, 64:], g[:, 64:], beta[:, 64:], state)
    prefill_within_bound(torch.cat([out, last], dim=1)[0], state[0], c, key)
    eager_state, graph_state = state.clone(), state.clone()
    eager = [step(q[:, 64:], k[:, 64:], v[:, 64:], g[:, 64:], beta[:, 64:], eager_state).clone() for _ in range(3)]
    warm = state.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(q[:, 64:], k[:, 64:], v[:, 64:], g[:, 64:], beta[:, 64:], warm)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step(q[:, 64:], k[:, 64:], v[:, 64:], g[:, 64:], beta[:, 64:], graph_state)
    graph_state.copy_(state)
    for i in range(3):
        graph.replay()
        assert torch.equal(captured, eager[i]), f"replay {i} differs from the eager call"
    assert torch.equal(graph_state, eager_state)
