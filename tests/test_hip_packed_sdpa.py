"""GPU parity of the packed var-len bidirectional attention (`MojoPackedSdpa`) through the C ABI.

Tolerance: atol = rtol = 2e-2 over every element, the bound tests/test_hip_sdpa.py applies to the same kernel family.  The oracle
is tests/vision_tower_golden.py on the CPU (pinned to the reference's ``MojoSWA(is_causal=False)`` by
tests/test_vision_tower_golden.py).  Sizes sit around the kernel's edges: the key tile is 64 keys, a workgroup owns 128 / G
query positions, and a forced key split of 3 cuts a block of >= 24 key tiles three ways.

Every case runs in three launch forms — unsplit, the key split forced (MOJO_HIP_PREFILL_KSPLIT) and general staging
(MOJO_HIP_PREFILL_FAST_STAGE=0) — and `mojo_hip_last_launch()` is asserted each time."""
import pytest
import torch

import vision_tower_golden as G
import visibility_sdpa as vis
from conftest import load_golden
from hip_utils import DEV, assert_close_tree, hip_cls, last_launch, run_hip_case, switch_env, to_cpu
from test_hip_sdpa import FORMS, dev

pytestmark = pytest.mark.gpu
ATOL = RTOL = 2e-2                   # tests/test_hip_sdpa.py's
NAME = "MojoPackedSdpa"
BF16, F16 = torch.bfloat16, torch.float16


def ops(layout="AABB"):
    return hip_cls(NAME)(gqa_layout=layout), G.TorchPackedSdpa(gqa_layout=layout)


def cumulative(lens, first=0):
    return torch.tensor([first] + [first + sum(lens[:i + 1]) for i in range(len(lens))], dtype=torch.int32)


def packed(g, hq, hkv, d, dtype, q_lens, kv_lens, first=0, q_pad=0, kv_pad=0):
    q = torch.randn(sum(q_lens) + q_pad, hq, d, generator=g).to(dtype)
    k = torch.randn(first + sum(kv_lens) + kv_pad, hkv, d, generator=g).to(dtype)
    v = torch.randn(first + sum(kv_lens) + kv_pad, hkv, d, generator=g).to(dtype)
    return q, k, v, cumulative(q_lens), cumulative(kv_lens, first)


def on_gpu(op, q, k, v, cu_q, cu_kv, scale=None, **hints):
    out = op.forward(dev(q), dev(k), dev(v), cu_q.to(DEV), cu_kv.to(DEV), scale, **hints)
    torch.cuda.synchronize()
    return out


def expect_tag(stage, ksplit):
    want = f"packed_sdpa:default:{stage}:ksplit{ksplit}"
    assert last_launch() == want, (last_launch(), want)


def in_every_form(hip, args, want, scale=None, **hints):
    outs = []
    for env, stage, ksplit in FORMS:
        with switch_env(**env):
            got = on_gpu(hip, *args, scale, **hints)
            expect_tag(stage, ksplit)
        outs.append(to_cpu(got))
        assert_close_tree(outs[-1], want, ATOL, RTOL)
    return outs


@pytest.mark.parametrize("case", [pytest.param(c, id=f"{i}-{c['ctor']['kwargs']['gqa_layout']}")
                                  for i, c in enumerate(load_golden("vision_tower")) if c["op"] == NAME])
def test_captured_vectors(case):
    assert_close_tree(to_cpu(run_hip_case(case)), case["out"], ATOL, RTOL)
    assert last_launch().startswith("packed_sdpa:default:")


KV_LENS = [1, 63, 64, 65, 128, 130, 1100]


def _edge_cases():
    cases = []
    for gi, grp in enumerate((1, 4, 8)):
        for vi, d in enumerate((64, 96, 128)):
            i = gi * 3 + vi
            cases.append(pytest.param(grp, d, (BF16, F16)[i % 2], ("AABB", "ABAB")[(i // 2) % 2], i % len(KV_LENS),
                                      id=f"G{grp}-D{d}-{('bf16', 'fp16')[i % 2]}-{('AABB', 'ABAB')[(i // 2) % 2]}-rot{i % len(KV_LENS)}"))
    return cases


@pytest.mark.parametrize("grp,d,dtype,layout,rot", _edge_cases())
def test_parity_around_every_edge_of_the_walk(grp, d, dtype, layout, rot):
    """One batch per case: q_len in {1, 128/G - 1, 128/G, 128/G + 1, 300} and every kv_len of KV_LENS, paired by a rotation that
    differs per case (q_len > kv_len and q_len < kv_len both occur in every batch), plus an empty-query sequence, a sequence
    without keys (rows exactly zero), cu_total_seq_lens[0] = 5 and 9 padding rows behind cu_q_lens[-1] (exactly zero)."""
    qpb = 128 // grp
    q_lens = [1, qpb - 1, qpb, qpb + 1, 300, 0, 7, 3]
    kv_lens = [KV_LENS[(j + rot) % len(KV_LENS)] for j in range(len(KV_LENS))] + [0]
    assert any(a > b > 0 for a, b in zip(q_lens, kv_lens)) and any(0 < a < b for a, b in zip(q_lens, kv_lens))
    hkv = 2 if grp < 8 else 1
    g = torch.Generator().manual_seed(100 * grp + d + rot)
    args = packed(g, hkv * grp, hkv, d, dtype, q_lens, kv_lens, first=5, q_pad=9, kv_pad=11)
    hip, ref = ops(layout)
    want = ref.forward(*args)
    cu_q = args[3].tolist()
    for got in in_every_form(hip, args, want):
        assert not bool(got[cu_q[-1]:].any()), "padding rows behind cu_q_lens[-1] must be zeros"
        assert not bool(got[cu_q[-2]:cu_q[-1]].any()), "rows of a sequence without keys must be zeros"
        assert bool(torch.isfinite(got.float()).all())


@pytest.mark.parametrize("grp,sq,sk,d,dtype,batch", [
    (1, 130, 65, 64, BF16, 1), (4, 33, 257, 128, F16, 1), (8, 17, 1600, 96, BF16, 1), (2, 70, 1700, 128, BF16, 1),
    (4, 40, 130, 64, BF16, 3), (1, 129, 1537, 128, F16, 2)])
def test_same_bits_as_sdpa_on_the_same_tokens(grp, sq, sk, d, dtype, batch):
    """`batch` equal sequences of Sq x Sk against `HIPSdpa` with that batch on the same memory (contiguous, token-major), at an
    equal key split (forced), unsplit, split and with the general staging."""
    hkv = 2 if grp < 8 else 1
    hq = hkv * grp
    g = torch.Generator().manual_seed(sq + sk)
    q, k, v, cu_q, cu_kv = packed(g, hq, hkv, d, dtype, [sq] * batch, [sk] * batch)
    hip, _ = ops("AABB")
    sdpa = hip_cls("MojoSdpa")(enable_gqa=True)
    dq, dk, dv = q.to(DEV), k.to(DEV), v.to(DEV)
    for env, stage, ksplit in FORMS:
        with switch_env(**env):
            mine = hip.forward(dq, dk, dv, cu_q.to(DEV), cu_kv.to(DEV), max_q_len=sq, max_total_seq_len=sk)
            expect_tag(stage, ksplit)
            theirs = sdpa.forward(dq.view(batch, sq, hq, d).transpose(1, 2), dk.view(batch, sk, hkv, d).transpose(1, 2),
                                  dv.view(batch, sk, hkv, d).transpose(1, 2))
            assert last_launch() == f"sdpa:default:{stage}:ksplit{ksplit}"
            torch.cuda.synchronize()
        assert torch.equal(mine.view(batch, sq, hq, d), theirs.transpose(1, 2))


def _visibility_inputs(hq, hkv, d, dtype, q_lens, kv_lens, gap=70):
    """Q[..., 0] = 1, K = 0, scale 1: a row's weights are exactly 1 / kv_len over its own keys.  Channel c of V is a probe of real
    sequence c % n: 1 at one key of that sequence (vis.probe_keys: both sides of every tile and slice boundary, the ends), 0
    elsewhere.  Between two real sequences, in front of the first and behind cu_total_seq_lens[-1] sit `gap` poison rows —
    K[..., 0] = 256 (a leaked key takes all the weight), V = 1 on every channel — owned by sequences WITHOUT queries (the arrays
    are cumulative: a neighbour's rows always belong to some sequence)."""
    n = len(q_lens)
    all_q, all_kv = [], []
    for ql, kl in zip(q_lens, kv_lens):
        all_q += [ql, 0]
        all_kv += [kl, gap]
    cu_q, cu_kv = cumulative(all_q), cumulative(all_kv, gap)
    tq, tk = int(cu_q[-1]) + 6, int(cu_kv[-1]) + gap
    q = torch.zeros(tq, hq, d, dtype=dtype)
    q[..., 0] = 1
    k, v = torch.zeros(tk, hkv, d, dtype=dtype), torch.zeros(tk, hkv, d, dtype=dtype)
    k[..., 0], v[:] = 256, 1                                                 # poison everywhere ...
    want = torch.zeros(tq, hq, d, dtype=dtype)
    seen = torch.zeros(tq, hq, d, dtype=torch.bool)
    for b, (ql, kl) in enumerate(zip(q_lens, kv_lens)):
        k0, q0 = int(cu_kv[2 * b]), int(cu_q[2 * b])
        k[k0:k0 + kl], v[k0:k0 + kl] = 0, 0                                  # ... but in the real sequences' rows
        keys = vis.probe_keys(kl, d)
        for c in range(d):
            if c % n == b:
                v[k0 + keys[c], :, c] = 1
                seen[q0:q0 + ql, :, c] = True
        want[q0:q0 + ql] = torch.where(seen[q0:q0 + ql], torch.tensor(1.0 / kl, dtype=torch.float32), torch.tensor(0.0)).to(dtype)
    return (q, k, v, cu_q, cu_kv), want, seen


@pytest.mark.parametrize("grp,d,dtype,layout,q_lens,kv_lens", [
    (1, 64, BF16, "AABB", [130, 33, 5], [65, 130, 1600]), (4, 128, F16, "ABAB", [33, 70, 40], [1537, 63, 129]),
    (8, 96, BF16, "AABB", [17, 16, 15, 40], [64, 1, 1601, 191])])
def test_exact_visible_set(grp, d, dtype, layout, q_lens, kv_lens):
    """Every row of every sequence returns 1 / kv_len on exactly its own sequence's probes and exactly 0 on the others'; rows no
    sequence owns are zeros.  No row is left out."""
    hkv = 2 if grp < 8 else 1
    args, want, seen = _visibility_inputs(hkv * grp, hkv, d, dtype, q_lens, kv_lens)
    hip, ref = ops(layout)
    vis.compare(ref.forward(*args, 1.0), want, seen)                         # the construction itself, against the golden
    for env, stage, ksplit in FORMS:
        with switch_env(**env):
            got = on_gpu(hip, *args, 1.0)
            expect_tag(stage, ksplit)
        vis.compare(to_cpu(got), want, seen)


def test_kv_views_of_a_fused_qkv_buffer_are_read_in_place():
    g = torch.Generator().manual_seed(31)
    hq, hkv, d, dtype = 8, 2, 128, BF16
    lens = [70, 1, 130, 64]
    tokens, guard = sum(lens), 8
    whole = torch.full((tokens + 2 * guard, hq + 2 * hkv, d), float("nan"), dtype=dtype)   # NaN guard rows around the buffer
    whole[guard:guard + tokens] = torch.randn(tokens, hq + 2 * hkv, d, generator=g).to(dtype)
    fused = whole[guard:guard + tokens]
    q, k, v = fused[:, :hq], fused[:, hq:hq + hkv], fused[:, hq + hkv:]
    assert k.stride() == v.stride() and not k.is_contiguous()
    cu = cumulative(lens)
    hip, ref = ops()
    want = ref.forward(q, k, v, cu, cu)
    for got in in_every_form(hip, (q, k, v, cu, cu), want):
        assert bool(torch.isfinite(got.float()).all())
    in_place = to_cpu(on_gpu(hip, q, k, v, cu, cu))
    dense = to_cpu(on_gpu(hip, q.contiguous(), k.contiguous(), v.contiguous(), cu, cu))
    assert torch.equal(in_place, dense)


def test_bits_are_identical_run_to_run_and_a_captured_call_replays_them():
    g = torch.Generator().manual_seed(4)
    q, k, v, cu_q, cu_kv = packed(g, 8, 2, 128, BF16, [150, 20, 64], [1700, 65, 300], first=3, q_pad=5)
    hip, _ = ops("ABAB")
    dargs = (q.to(DEV), k.to(DEV), v.to(DEV), cu_q.to(DEV), cu_kv.to(DEV))
    for env, stage, ksplit in FORMS:
        with switch_env(**env):
            first = hip.forward(*dargs)
            again = hip.forward(*dargs)
            torch.cuda.synchronize()
            expect_tag(stage, ksplit)
            assert torch.equal(first, again)
    eager = hip.forward(*dargs)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        hip.forward(*dargs)                                  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = hip.forward(*dargs)
    captured.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured, eager)


def test_lengths_above_their_hints_behave_as_documented():
    """Rows past ``max_q_len`` of a sequence are zeros; keys at or past ``max_total_seq_len`` are not seen (the golden states
    both).  A call inside its hints has the bits of the call without them at the same key split."""
    g = torch.Generator().manual_seed(12)
    q_lens, kv_lens = [70, 20, 45], [130, 40, 100]
    args = packed(g, 4, 2, 64, F16, q_lens, kv_lens, q_pad=3)
    hip, ref = ops()
    hints = dict(max_q_len=40, max_total_seq_len=100)
    want = ref.forward(*args, **hints)
    cu_q = args[3].tolist()
    assert bool(want[cu_q[0]:cu_q[0] + 40].any()) and not bool(want[cu_q[0] + 40:cu_q[1]].any())
    for got in in_every_form(hip, args, want, **hints):
        assert not bool(got[cu_q[0] + 40:cu_q[1]].any()) and not bool(got[cu_q[2] + 40:cu_q[3]].any()) and not bool(got[cu_q[3]:].any())
    # keys past the hint are unseen, exactly: poison behind key 100 of sequence 0 changes nothing
    q, k, v, cu_q_t, cu_kv_t = args
    k2, v2 = k.clone(), v.clone()
    k2[100:130], v2[100:130] = 256, 1000
    with switch_env(MOJO_HIP_PREFILL_KSPLIT="1"):
        a = to_cpu(on_gpu(hip, q, k, v, cu_q_t, cu_kv_t, **hints))
        b = to_cpu(on_gpu(hip, q, k2, v2, cu_q_t, cu_kv_t, **hints))
        loose = to_cpu(on_gpu(hip, q, k, v, cu_q_t, cu_kv_t, max_q_len=70, max_total_seq_len=130))
        bare = to_cpu(on_gpu(hip, q, k, v, cu_q_t, cu_kv_t))
    assert torch.equal(a, b) and torch.equal(loose, bare)


def test_the_envelope_raises():
    hip, _ = ops()
    cu = torch.tensor([0, 4], dtype=torch.int32, device=DEV)

    def call(hq, hkv, d, dtype):
        return hip.forward(torch.zeros(4, hq, d, dtype=dtype, device=DEV), torch.zeros(4, hkv, d, dtype=dtype, device=DEV),
                           torch.zeros(4, hkv, d, dtype=dtype, device=DEV), cu, cu)

    with pytest.raises(NotImplementedError, match="head_dim 80"):
        call(4, 4, 80, BF16)
    with pytest.raises(NotImplementedError, match="3 query heads"):
        call(6, 2, 64, BF16)
    with pytest.raises(NotImplementedError, match="float32"):
        call(4, 4, 64, torch.float32)
    assert call(4, 4, 64, BF16).shape == (4, 4, 64)
