"""GPU parity of the W8A8 MoE ops (`MojoMoEDynamicQuant`, `MojoQuantExperts`, `MojoQuantMoE`) against oracle/quant_moe.py.

* the quantiser and the grouped int8 product are BIT-EXACT (atol = rtol = 0): products and divisions are the IEEE single
  operations, int32 accumulation is exact and associative, so every kernel form, tile shape and K split gives the golden's bits
  (the `exact_int` form of the golden, whose 2**24 bound every test asserts on its own data);
* the SwiGLU-quantise kernel is judged by the reference's bounds for this kernel family (|dq| <= 1, scale rtol 2e-3:
  mojo_opset/tests/accuracy/operators/test_moe_quant.py:203, test_quantize.py:222) and by the bound that follows from the
  arithmetic, |q * s - y| <= s (half a step for the rounding, half a step of slack for the device's exp and the row scale);
* the experts and the layer by the reference's own criterion, `mixed_tol` (test_moe_quant.py:281, :353), on weights drawn as
  randn * 0.1 so that at least half of the golden's outputs have |ref| >= 1 (asserted).
"""
import pytest
import torch

import oracle.quant_moe as G
from conftest import bit_equal, build_op, clone_tree, load_golden
from hip_utils import DEV, hip_cls, last_launch, launches_of, run_hip_case, switch_env, to_cpu
from mojo_opset_amd.backends.hip.operators.moe import HIPQuantExperts
from mojo_opset_amd.backends.hip.operators.quantize import moe_dynamic_quant as hip_moe_quant
from mojo_opset_amd.core import check_tol_diff

pytestmark = pytest.mark.gpu

CASES = load_golden("quant_moe")
QUANT = [c for c in CASES if c["op"] == "MojoMoEDynamicQuant"]
EXPERTS = [c for c in CASES if c["op"] == "MojoQuantExperts" and "up_weight_dtype" not in c["ctor"]["kwargs"]]
LAYER = [c for c in CASES if c["op"] == "MojoQuantMoE"]

NO_RAGGED = "29"          # MOJO_HIP_GEMM_SKINNY without bit 2 (the ragged weight stream)


def _ids(cases, tag):
    return [pytest.param(c, id=f"{tag}-{i}") for i, c in enumerate(cases)]


def quantize_rows(x, q_max=127.0):
    """Per-row amax / 127 quantisation: the data the experts' projections really see."""
    scale = (x.float().abs().amax(dim=-1, keepdim=True) / q_max).clamp(min=1e-12)
    return torch.round(x.float() / scale).clamp(-128, 127).to(torch.int8), scale


def ep_counts(experts, tokens, top_k, dtype=torch.int32, seed=0):
    """The reference test's counts: ids over 2 * experts with the upper half dropped (the EP case)."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, 2 * experts, (tokens, top_k), generator=g)
    return torch.bincount(ids.flatten(), minlength=2 * experts)[:experts].to(dtype)


# ---- 1. HIPMoEDynamicQuant ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", _ids(QUANT, "quant"))
def test_quantiser_vectors_bit_exact(case):
    assert bit_equal(to_cpu(run_hip_case(case)), case["out"])


@pytest.mark.parametrize("tokens,hidden,counts", [(8, 128, [8]), (12, 256, [4, 3, 5]), (18, 512, [6, 6, 4, 2]),
                                                  (21, 1024, [2, 5, 1, 7, 6]), (32, 2048, [8, 7, 5, 6, 4, 2]),
                                                  (40, 7168, [0, 13, 0, 27, 0]),          # empty experts
                                                  (9, 10240, [4, 0, 5]),                  # rows longer than the registers hold (16-bit: > 8192)
                                                  (7, 100, [3, 4])])                      # no 16-byte vectors
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("cdtype", [torch.int32, torch.int64])
def test_quantiser_reference_space_bit_exact(tokens, hidden, counts, dtype, cdtype):
    torch.manual_seed(tokens + hidden)
    x = torch.randn(tokens, hidden).to(dtype)
    cnt = torch.tensor(counts, dtype=cdtype)
    inv = 1.0 / (torch.rand(len(counts), hidden) + 0.1)
    ref = G.TorchMoEDynamicQuant(len(counts), hidden)
    op = hip_cls("MojoMoEDynamicQuant")(len(counts), hidden).to(DEV)
    with torch.no_grad():
        ref.inv_smooth_scale.copy_(inv)
        op.inv_smooth_scale.copy_(inv)
    want_q, want_s = ref(x, cnt)
    got_q, got_s = op(x.to(DEV), cnt.to(DEV))
    torch.testing.assert_close(to_cpu(got_q), want_q, atol=0, rtol=0)
    torch.testing.assert_close(to_cpu(got_s), want_s, atol=0, rtol=0)
    wide = hidden % (16 // x.element_size()) == 0             # 16-byte loads: eight 16-bit or four fp32 elements
    assert last_launch() == "moe_quant:plain:" + ("vec16" if wide else "scalar")


def test_quantiser_rows_past_the_counts_and_leading_dimensions():
    torch.manual_seed(3)
    x = torch.randn(2, 6, 256).to(torch.bfloat16)                 # [*, K]: 12 rows, the counts cover 9
    cnt = torch.tensor([4, 0, 5], dtype=torch.int32)
    op = hip_cls("MojoMoEDynamicQuant")(3, 256).to(DEV)
    with torch.no_grad():
        op.inv_smooth_scale.copy_(torch.rand(3, 256) + 0.5)
    q, s = (to_cpu(t) for t in op(x.to(DEV), cnt.to(DEV)))
    assert q.shape == (2, 6, 256) and s.shape == (2, 6, 1)
    want_q, want_s = G.moe_dynamic_quant(x.reshape(12, 256)[:9], op.inv_smooth_scale.detach().cpu(), cnt)
    assert torch.equal(q.reshape(12, 256)[:9], want_q) and torch.equal(s.reshape(12, 1)[:9], want_s)
    assert not q.reshape(12, 256)[9:].any() and torch.equal(s.reshape(12, 1)[9:], torch.ones(3, 1))


# ---- 2. the grouped quantised GEMM ---------------------------------------------------------------------------------------

def _gemm(x8, xs, w8, ws, counts, dtype):
    out = HIPQuantExperts._group_quant_gemm(x8.to(DEV), xs.to(DEV), w8.to(DEV), ws.to(DEV), counts.to(DEV), dtype)
    torch.cuda.synchronize()
    return to_cpu(out)


def _gemm_golden(x8, xs, w8, ws, counts, dtype):
    """The experts' quant-linear per group, `exact_int` (asserts sum |x||w| < 2**24 on this data); rows past the counts are zero."""
    out = torch.zeros(x8.shape[0], w8.shape[1], dtype=dtype)
    at = 0
    for g, n in enumerate(counts.tolist()):
        n = min(n, x8.shape[0] - at)
        if n > 0:
            out[at:at + n] = G.quant_linear(x8[at:at + n], xs[at:at + n], w8[g], ws[g], dtype, exact_int=True)
        at += n
    return out


def _gemm_data(groups, k, n, rows, full_range, seed=0):
    g = torch.Generator().manual_seed(seed)
    if full_range:                                             # any int8 data: K <= 512 keeps 128 * 128 * K below 2**24
        assert k * 128 * 128 < G.EXACT_BOUND
        x8 = torch.randint(-128, 128, (rows, k), generator=g, dtype=torch.int8)
        w8 = torch.randint(-128, 128, (groups, n, k), generator=g, dtype=torch.int8)
        xs = torch.rand(rows, 1, generator=g) * 0.02 + 0.001
    else:
        x8, xs = quantize_rows(torch.randn(rows, k, generator=g))
        w8 = quantize_rows(torch.randn(groups, n, k, generator=g) * 0.1)[0]
    ws = (torch.rand(groups, n, generator=g) * 0.01 + 0.0005).to(torch.bfloat16)
    return x8, xs, w8, ws


TILE_LEGS = [("256", dict(MOJO_HIP_GEMM_TILE128="0", MOJO_HIP_GEMM_SPLITK="1"), "group_quant256:"),
             ("tile128", dict(MOJO_HIP_GEMM_TILE128="1", MOJO_HIP_GEMM_SPLITK=None), "group_quant_tile128:gemm128:"),
             ("tile128x256", dict(MOJO_HIP_GEMM_TILE128="256", MOJO_HIP_GEMM_SPLITK=None), "group_quant_tile128:gemm128:128x256"),
             ("splitk", dict(MOJO_HIP_GEMM_TILE128="0", MOJO_HIP_GEMM_SPLITK="3"), "group_quant256:splitk3"),
             ("default", dict(MOJO_HIP_GEMM_TILE128=None, MOJO_HIP_GEMM_SPLITK=None), "group_quant")]


@pytest.mark.parametrize("groups,k,n,counts,full_range", [
    (4, 512, 512, [300, 0, 700, 260], True),                   # full-range int8, an empty group, partial tiles
    (3, 2048, 384, [129, 1, 511], False),                      # N not a multiple of 256, a one-row group
    (2, 7168, 256, [200, 150], False),                         # the longest K of the bench shapes
    (5, 384, 1024, [0, 0, 640, 0, 0], True),                   # one group holds every row
])
@pytest.mark.parametrize("dtype,cdtype", [(torch.bfloat16, torch.int32), (torch.float16, torch.int64), (torch.float32, torch.int32)])
def test_group_gemm_tile_forms_bit_exact_and_identical(groups, k, n, counts, full_range, dtype, cdtype):
    cnt = torch.tensor(counts, dtype=cdtype)
    rows = int(cnt.sum()) + 5                                   # five rows past sum(counts): they must read zero
    x8, xs, w8, ws = _gemm_data(groups, k, n, rows, full_range, seed=k + n)
    want = _gemm_golden(x8, xs, w8, ws, cnt, dtype)
    assert not want[int(cnt.sum()):].any()
    for name, env, note in TILE_LEGS:
        with switch_env(MOJO_HIP_GEMM_SKINNY=NO_RAGGED, **env):
            got = _gemm(x8, xs, w8, ws, cnt, dtype)
            assert last_launch().startswith(note), (name, last_launch())
        assert torch.equal(got, want), f"{name} ({last_launch()}): {(got.float() - want.float()).abs().max()}"


@pytest.mark.parametrize("groups,k,n,counts", [
    (8, 512, 256, [3, 0, 17, 1, 40, 0, 9, 16]),                # mean <= 16 rows: 16-row tiles, a group of three tiles
    (4, 7168, 128, [20, 31, 0, 33]),                           # 32-row tiles at the longest K
    (3, 1024, 192, [64, 50, 60]),                              # 64-row tiles
    (64, 256, 64, [8] * 64),                                   # the decode layer's shape of counts
])
@pytest.mark.parametrize("dtype,cdtype", [(torch.bfloat16, torch.int64), (torch.float16, torch.int32), (torch.float32, torch.int32)])
def test_group_gemm_ragged_decode_form_bit_exact_and_identical_to_the_tiles(groups, k, n, counts, dtype, cdtype):
    cnt = torch.tensor(counts, dtype=cdtype)
    rows = int(cnt.sum()) + 2
    x8, xs, w8, ws = _gemm_data(groups, k, n, rows, k <= 512, seed=groups + k)
    want = _gemm_golden(x8, xs, w8, ws, cnt, dtype)
    got = _gemm(x8, xs, w8, ws, cnt, dtype)
    assert last_launch().startswith("group_quant_ragged:rows"), last_launch()
    assert torch.equal(got, want)
    with switch_env(MOJO_HIP_GEMM_SKINNY=NO_RAGGED):
        tiles = _gemm(x8, xs, w8, ws, cnt, dtype)
        assert last_launch().startswith(("group_quant_tile128:", "group_quant256:")), last_launch()
    assert torch.equal(tiles, want)


@pytest.mark.parametrize("groups,k,n,counts", [(3, 100, 50, [7, 0, 30]), (2, 257, 64, [65, 3]), (2, 128, 7, [10, 10])])
def test_group_gemm_generic_fallback_for_odd_shapes(groups, k, n, counts):
    cnt = torch.tensor(counts, dtype=torch.int32)
    x8, xs, w8, ws = _gemm_data(groups, k, n, int(cnt.sum()) + 1, True, seed=k)
    got = _gemm(x8, xs, w8, ws, cnt, torch.bfloat16)
    assert last_launch() == "group_quant_generic"
    assert torch.equal(got, _gemm_golden(x8, xs, w8, ws, cnt, torch.bfloat16))


def test_group_gemm_zero_rows_in_total():
    x8, xs, w8, ws = _gemm_data(3, 256, 128, 6, True)
    out = _gemm(x8, xs, w8, ws, torch.zeros(3, dtype=torch.int32), torch.bfloat16)      # counts all zero: every row is a trailing row
    assert out.shape == (6, 128) and not out.any()
    empty = _gemm(x8[:0], xs[:0], w8, ws, torch.zeros(3, dtype=torch.int64), torch.float16)
    assert empty.shape == (0, 128)


def test_group_gemm_bench_sized_first_projection_on_sampled_rows():
    """E 8 / H 4096 / I 14336, 16384 rows (T 8192 x top-2): the bench's first projection, a few rows of every expert against
    the CPU golden."""
    groups, k, n, rows = 8, 4096, 2 * 14336, 16384
    g = torch.Generator(device=DEV).manual_seed(5)
    counts = torch.tensor([2048, 1500, 2596, 2048, 100, 3996, 2048, 2048], dtype=torch.int32)
    assert int(counts.sum()) == rows
    x8, xs = quantize_rows(torch.randn(rows, k, generator=g, device=DEV))
    w8 = torch.empty(groups, n, k, dtype=torch.int8, device=DEV)
    for e in range(groups):
        w8[e] = quantize_rows(torch.randn(n, k, generator=g, device=DEV) * 0.1)[0]
    ws = (torch.rand(groups, n, generator=g, device=DEV) * 0.01 + 0.0005).to(torch.bfloat16)
    out = HIPQuantExperts._group_quant_gemm(x8, xs, w8, ws, counts.to(DEV), torch.bfloat16)
    torch.cuda.synchronize()
    assert last_launch().startswith("group_quant256:"), last_launch()
    ends = counts.cumsum(0).tolist()
    for e in range(groups):
        lo, hi = ends[e] - int(counts[e]), ends[e]
        pick = torch.tensor(sorted({lo, (lo + hi) // 2, hi - 1}))
        want = G.quant_linear(x8[pick.to(DEV)].cpu(), xs[pick.to(DEV)].cpu(), w8[e].cpu(), ws[e].cpu(), torch.bfloat16, exact_int=True)
        assert torch.equal(out[pick.to(DEV)].cpu(), want), f"expert {e}"


# ---- 3. dequantised fc1 -> SwiGLU -> smooth -> quantise --------------------------------------------------------------------

def _experts_pair(experts, hidden, inter, dtype, seed=0):
    """Golden and hip experts with the reference test's state, weights drawn as randn * 0.1."""
    g = torch.Generator().manual_seed(seed)
    up8, up_s = quantize_rows(torch.randn(experts, 2 * inter, hidden, generator=g) * 0.1)
    down8, down_s = quantize_rows(torch.randn(experts, hidden, inter, generator=g) * 0.1)
    state = {"up_proj_weight": up8, "down_proj_weight": down8, "up_proj_weight_scale": up_s.squeeze(-1).bfloat16(),
             "down_proj_weight_scale": down_s.squeeze(-1).bfloat16(),
             "up_proj_quantize.inv_smooth_scale": 1.0 / (torch.rand(experts, hidden, generator=g) + 0.5),
             "down_proj_quantize.inv_smooth_scale": 1.0 / (torch.rand(experts, inter, generator=g) + 0.5)}
    ref = G.TorchQuantExperts(experts, hidden, inter)
    ref.exact_int = True
    op = hip_cls("MojoQuantExperts")(experts, hidden, inter).to(DEV)
    ref.load_state_dict(state)
    op.load_state_dict(state)
    return ref, op, g


@pytest.mark.parametrize("experts,hidden,inter,tokens,top_k", [(16, 512, 1280, 33, 2), (24, 512, 1280, 97, 4), (4, 128, 192, 40, 2)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_swiglu_quantise_kernel_on_the_goldens_own_fc1(experts, hidden, inter, tokens, top_k, dtype):
    ref, op, g = _experts_pair(experts, hidden, inter, dtype, seed=experts)
    cnt = ep_counts(experts, tokens, top_k)
    x = torch.randn(int(cnt.sum()), hidden, generator=g).to(dtype)
    with torch.no_grad():
        _, _, fc1, _, smoothed, want_q, want_s, _ = ref.stages(x, cnt)
    q, s = hip_moe_quant(fc1.to(DEV), op.down_proj_quantize.inv_smooth_scale.detach(), cnt.to(DEV), inter, True, "test")
    torch.cuda.synchronize()
    assert last_launch().startswith("moe_quant:swiglu:vec16")
    q, s = to_cpu(q), to_cpu(s)
    differ = (q != want_q).float().mean().item()
    print(f"swiglu-quantise E{experts} H{hidden} I{inter} {dtype}: {differ:.3%} of {q.numel()} int8 elements differ from the golden, "
          f"max scale error {((s - want_s).abs() / want_s).max().item():.3g} relative")
    assert (q.int() - want_q.int()).abs().max().item() <= 1
    torch.testing.assert_close(s, want_s, atol=0, rtol=2e-3)
    assert bool(((q.float() * s - smoothed).abs() <= s).all())


# ---- 4. HIPQuantExperts end to end -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", _ids(EXPERTS, "experts"))
def test_experts_vectors(case):
    check_tol_diff(to_cpu(run_hip_case(case)), case["out"], mixed_tol=True)


@pytest.mark.parametrize("experts,top_k,hidden,inter,tokens", [(16, 2, 512, 1280, 33), (24, 4, 512, 1280, 97)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("ragged", [True, False])
def test_experts_reference_space(experts, top_k, hidden, inter, tokens, dtype, ragged):
    ref, op, g = _experts_pair(experts, hidden, inter, dtype, seed=tokens)
    cnt = ep_counts(experts, tokens, top_k)
    x = torch.randn(int(cnt.sum()), hidden, generator=g).to(dtype)
    with torch.no_grad():
        x8, _, _, _, _, y8, _, want = ref.stages(x, cnt)
    ends = cnt.cumsum(0).tolist()
    for e in range(experts):                                   # the 2**24 bound of the exact_int golden, on this data
        lo, hi = ends[e] - int(cnt[e]), ends[e]
        assert G.dot_bound(x8[lo:hi], ref.up_proj_weight[e]) < G.EXACT_BOUND and G.dot_bound(y8[lo:hi], ref.down_proj_weight[e]) < G.EXACT_BOUND
    assert (want.float().abs() >= 1).float().mean().item() >= 0.5, "the golden's outputs must exercise the rtol branch of mixed_tol"
    with switch_env(MOJO_HIP_GEMM_SKINNY=None if ragged else NO_RAGGED):
        notes = launches_of(lambda: op(x.to(DEV), cnt.to(DEV)))
        got = op(x.to(DEV), cnt.to(DEV))
        again = op(x.to(DEV), cnt.to(DEV))
        torch.cuda.synchronize()
    assert ("group_quant_ragged" in notes) == ragged and "moe_quant:swiglu" in notes and "moe_quant:plain" in notes, notes
    assert torch.equal(got, again)
    same = (to_cpu(got) == want).float().mean().item()
    print(f"experts E{experts} k{top_k} T{tokens} {dtype} {'ragged' if ragged else 'tiles'}: {same:.3%} of outputs bit-equal to the golden; |ref| max {want.float().abs().max():.1f}")
    check_tol_diff(to_cpu(got), want, mixed_tol=True)


@pytest.mark.parametrize("counts,extra", [([8] * 16, 0),                       # a decode-shaped count vector
                                          ([5, 0, 0, 70, 1, 0, 130, 2], 0),      # empty experts, more than a tile of rows
                                          ([3, 4, 0, 9], 6),                     # trailing rows past sum(counts)
                                          ([0, 0, 0, 0], 5),                     # no expert has a row
                                          ([0, 0], 0)])                          # zero rows
def test_experts_count_shapes(counts, extra):
    experts = len(counts)
    ref, op, g = _experts_pair(experts, 256, 384, torch.bfloat16, seed=experts + extra)
    cnt = torch.tensor(counts, dtype=torch.int64)
    live = int(cnt.sum())
    x = torch.randn(live + extra, 256, generator=g).to(torch.bfloat16)
    got = to_cpu(op(x.to(DEV), cnt.to(DEV)))
    assert got.shape == x.shape and not got[live:].any()
    if live:
        with torch.no_grad():
            want = ref(x[:live], cnt)
        check_tol_diff(got[:live], want, mixed_tol=True)


# ---- 5. HIPQuantMoE -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", _ids(LAYER, "layer"))
def test_layer_vectors(case):
    check_tol_diff(to_cpu(run_hip_case(case)), case["out"], mixed_tol=True)


def _layer_pair(experts, top_k, hidden, inter, seed):
    ref_e, _, g = _experts_pair(experts, hidden, inter, torch.bfloat16, seed=seed)
    state = {"experts." + k: v for k, v in ref_e.state_dict().items()}
    state["gating.gate_weight"] = torch.randn(hidden, experts, generator=g) * 0.2
    ref = G.TorchQuantMoE(experts, top_k, hidden, inter)
    ref.experts.exact_int = True
    op = hip_cls("MojoQuantMoE")(experts, top_k, hidden, inter).to(DEV)
    ref.load_state_dict(state)
    op.load_state_dict(state)
    return ref, op, g


@pytest.mark.parametrize("experts,top_k,hidden,inter,tokens", [(16, 2, 512, 1280, 33), (24, 4, 512, 1280, 97)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_layer_reference_space(experts, top_k, hidden, inter, tokens, dtype):
    ref, op, g = _layer_pair(experts, top_k, hidden, inter, seed=tokens + 1)
    assert type(op.experts) is hip_cls("MojoQuantExperts") and type(op.gating) is hip_cls("MojoMoEGating")
    x = torch.randn(tokens, hidden, generator=g).to(dtype)
    with torch.no_grad():
        want = ref(x)
    check_tol_diff(to_cpu(op(x.to(DEV))), want, mixed_tol=True)


# ---- 6. graph capture -----------------------------------------------------------------------------------------------------

def _capture(fn, warmup=2):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(warmup):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                             # a host sync anywhere in fn makes the capture fail
        out = fn()
    return graph, out


def test_experts_and_layer_replay_after_inputs_change_in_place():
    experts, top_k, hidden, inter, tokens = 16, 2, 512, 1280, 48
    _, ffn, g = _experts_pair(experts, hidden, inter, torch.bfloat16, seed=11)
    _, layer, _ = _layer_pair(experts, top_k, hidden, inter, seed=12)
    rows = tokens * top_k
    x_rows = torch.zeros(rows, hidden, dtype=torch.bfloat16, device=DEV)
    counts = torch.zeros(experts, dtype=torch.int32, device=DEV)
    x_tok = torch.zeros(tokens, hidden, dtype=torch.bfloat16, device=DEV)

    def fill(seed):
        gen = torch.Generator().manual_seed(seed)
        x_rows.copy_(torch.randn(rows, hidden, generator=gen))
        x_tok.copy_(torch.randn(tokens, hidden, generator=gen))
        ids = torch.randint(0, experts, (rows,), generator=gen)
        counts.copy_(torch.bincount(ids, minlength=experts).to(torch.int32))

    def step():                                                # one chain: the experts, then the layer
        return ffn(x_rows, counts), layer(x_tok)

    fill(0)
    graph, static_out = _capture(step)
    for i in range(3):
        fill(20 + i)
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in static_out]
        want = step()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(got, want))
