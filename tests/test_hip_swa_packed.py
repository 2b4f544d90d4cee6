"""GPU parity of the packed var-len attention over contiguous K/V (`MojoSWA`) through the C ABI.

Tolerance: atol = rtol = 2e-2, the reference's own bound for this operator (tests/accuracy/operators/test_attention.py
:2067-2068).  The oracle is tests/swa_packed_golden.py on CPU (pinned to the reference by tests/test_swa_packed_golden.py).
The EXACT tests compare with the paged prefill ops on the same tokens: the linear instances share the tile loop and its
arithmetic with the paged ones, so at the same key split the bits must be the same."""
import pytest
import torch

import swa_packed_golden
from conftest import load_golden
from hip_utils import DEV, assert_close_tree, hip_cls, last_launch, run_hip_case, switch_env, to_cpu
from swa_packed_utils import cumulative, packed_inputs, scatter_to_pages

pytestmark = pytest.mark.gpu
ATOL = RTOL = 2e-2
NAME = "MojoSWA"


def ops(layout="AABB", glob=None, local=None):
    kw = dict(gqa_layout=layout, global_window_size=glob, local_window_size=local)
    return hip_cls(NAME)(**kw), swa_packed_golden.TorchSWA(**kw)


def on_gpu(op, args, **kw):
    out = op.forward(*[a.to(DEV) if isinstance(a, torch.Tensor) else a for a in args], **kw)
    torch.cuda.synchronize()
    return out


def expect_tag(glob, local):
    form = last_launch()
    assert form.startswith("prefill_linear:default:"), form
    assert form.endswith(":swa") == (glob is not None or local is not None), form
    return form


def check(layout, glob, local, kv_lens, q_lens, **shape):
    args = packed_inputs(kv_lens, q_lens, **shape)
    hip, ref = ops(layout, glob, local)
    got = on_gpu(hip, args)
    expect_tag(glob, local)
    assert_close_tree(to_cpu(got), ref.forward(*args), ATOL, RTOL)
    return got


@pytest.mark.parametrize("case", [pytest.param(c, id=str(i)) for i, c in enumerate(load_golden("swa_packed"))])
def test_captured_vectors(case):
    assert_close_tree(to_cpu(run_hip_case(case)), case["out"], ATOL, RTOL)
    kw = case["ctor"]["kwargs"]
    expect_tag(kw["global_window_size"], kw["local_window_size"])


# the reference's config space (test_attention.py:2002-2006: batch, q heads, kv heads, head_dim, max q_len, max cached len) under
# both of its window / layout pairs (:2026-2029); lengths drawn as generate_sdpa_data draws them (:1979-1988)
CFGS = [(2, 16, 4, 128, 1024, 0), (2, 16, 4, 96, 1024, 0), (2, 8, 1, 128, 1024, 2048)]


@pytest.mark.parametrize("layout,glob,local", [("ABAB", 4, 255), ("AABB", 4, 1023)])
@pytest.mark.parametrize("cfg", CFGS, ids=lambda c: "x".join(map(str, c)))
def test_reference_config_space(cfg, layout, glob, local):
    batch, hq, hkv, d, max_q, max_cached = cfg
    g = torch.Generator().manual_seed(hq + d + max_cached)
    q_lens = torch.randint(max_q // 2, max_q, (batch,), generator=g).clamp(min=1)
    kv_lens = q_lens + (torch.randint(max_cached // 2, max_cached, (batch,), generator=g) if max_cached > 0 else 0)
    check(layout, glob, local, kv_lens.tolist(), q_lens.tolist(), hq=hq, hkv=hkv, d=d)


# sequence starts fall off every alignment; an empty sequence, a one-token one, chunks against a cached prefix
EXACT_KV, EXACT_Q = [77, 1, 130, 0, 63, 64, 65, 300], [77, 1, 30, 0, 63, 1, 65, 200]


@pytest.mark.parametrize("ksplit", ["1", "4"])
@pytest.mark.parametrize("page", [16, 64])
@pytest.mark.parametrize("layout,glob,local,paged_name", [("AABB", 4, 63, "MojoPagedPrefillSWA"), ("ABAB", None, 100, "MojoPagedPrefillSWA"),
                                                          ("AABB", None, None, "MojoPagedPrefillGQA")])
def test_exact_the_linear_launch_equals_the_paged_one(layout, glob, local, paged_name, page, ksplit):
    q, k, v, cu_q, cu_kv = packed_inputs(EXACT_KV, EXACT_Q, hq=8, hkv=2, d=128, seed=3)
    kc, vc, table, cu0 = scatter_to_pages(k, v, cu_kv, page)
    lin = ops(layout, glob, local)[0]
    if paged_name == "MojoPagedPrefillGQA":
        paged = hip_cls(paged_name)(gqa_layout=layout)
    else:
        paged = hip_cls(paged_name)(gqa_layout=layout, global_window_size=glob, local_window_size=local)
    with switch_env(MOJO_HIP_PREFILL_KSPLIT=ksplit):
        got = on_gpu(lin, (q, k, v, cu_q, cu_kv))
        form = expect_tag(glob, local)
        want = on_gpu(paged, (q, kc, vc, cu_q, table), cu_total_seq_lens=cu0.to(DEV))
        paged_form = last_launch()
    assert f":ksplit{ksplit}" in form and f":ksplit{ksplit}" in paged_form and paged_form.startswith("prefill:default:"), (form, paged_form)
    assert torch.equal(got, want)
    assert_close_tree(to_cpu(got), ops(layout, glob, local)[1].forward(q, k, v, cu_q, cu_kv), ATOL, RTOL)


@pytest.mark.parametrize("glob,local", [(None, None), (4, 1023)], ids=["plain", "swa"])
@pytest.mark.parametrize("env", [dict(MOJO_HIP_PREFILL_KSPLIT="1"), dict(MOJO_HIP_PREFILL_KSPLIT="4"),
                                 dict(MOJO_HIP_PREFILL_FAST_STAGE="0")], ids=lambda e: ",".join(e.values()))
def test_every_form(env, glob, local):
    with switch_env(**env):
        check("AABB", glob, local, [6000], [128], hq=8, hkv=2)
        form = expect_tag(glob, local)
    if "MOJO_HIP_PREFILL_KSPLIT" in env:
        assert f":ksplit{env['MOJO_HIP_PREFILL_KSPLIT']}" in form and ":fast_stage:" in form, form
    else:
        assert ":general_stage:" in form, form


@pytest.mark.parametrize("w", [1, 15, 16, 17, 63, 64, 65, 127])
def test_window_edges(w):
    """Local and global windows whose edges fall on, one short of and one past tile boundaries."""
    check("AABB", w, w, [400, 128 + w], [200, 100], hq=4, hkv=2, d=128)
    check("ABAB", None, w, [400, 128 + w], [200, 100], hq=2, hkv=2, d=64)
    check("AABB", w, 0, [400, 128 + w], [200, 100], hq=4, hkv=2, d=64)
    check("ABAB", w, w, [400, 128 + w], [200, 100], hq=2, hkv=2, d=128)


def fused_qkv(kv_lens, hq, hkv, d, dtype=torch.bfloat16, seed=5):
    """K and V as views of one fused [T, (Hq + 2 Hkv) * D] projection output (a first prefill: q_len == kv_len)."""
    g = torch.Generator().manual_seed(seed)
    tokens = sum(kv_lens)
    fused = torch.randn(tokens, (hq + 2 * hkv) * d, generator=g).to(dtype).to(DEV)
    q = fused[:, : hq * d].view(tokens, hq, d)
    k = fused[:, hq * d: (hq + hkv) * d].view(tokens, hkv, d)
    v = fused[:, (hq + hkv) * d:].view(tokens, hkv, d)
    cu = cumulative(kv_lens).to(DEV)
    return q, k, v, cu


@pytest.mark.parametrize("glob,local", [(None, None), (4, 100)], ids=["plain", "swa"])
def test_exact_views_of_a_fused_qkv_buffer_give_the_bits_of_contiguous_copies(glob, local):
    q, k, v, cu = fused_qkv([300, 77, 130], hq=8, hkv=2, d=128)
    assert not k.is_contiguous() and k.stride() == v.stride() and k.stride(0) == 12 * 128
    hip, ref = ops("AABB", glob, local)
    got = on_gpu(hip, (q, k, v, cu, cu))
    expect_tag(glob, local)
    assert torch.equal(got, on_gpu(hip, (q.contiguous(), k.contiguous(), v.contiguous(), cu, cu)))
    want = ref.forward(q.cpu(), k.cpu(), v.cpu(), cu.cpu(), cu.cpu())
    assert_close_tree(to_cpu(got), want, ATOL, RTOL)
    # K a view, V contiguous: different strides, so both are copied — still correct
    got2 = on_gpu(hip, (q, k, v.contiguous(), cu, cu))
    assert torch.equal(got2, got)


def test_a_positive_first_offset_and_unused_tokens_at_both_ends():
    q, k, v, cu_q, cu_kv = packed_inputs([90, 33, 200], [90, 3, 70], hq=8, hkv=2, d=128, lead=5, tail=9, seed=7)
    assert int(cu_kv[0]) == 5 and int(cu_kv[-1]) == k.shape[0] - 9
    for glob, local in [(None, None), (4, 63)]:
        hip, ref = ops("AABB", glob, local)
        want = ref.forward(q, k, v, cu_q, cu_kv)
        assert_close_tree(to_cpu(on_gpu(hip, (q, k, v, cu_q, cu_kv))), want, ATOL, RTOL)
        # what the unused tokens hold never reaches the output
        k2, v2 = k.clone(), v.clone()
        for t in (k2, v2):
            t[:5] = float("nan")
            t[-9:] = float("nan")
        assert_close_tree(to_cpu(on_gpu(hip, (q, k2, v2, cu_q, cu_kv))), want, ATOL, RTOL)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_zeros_and_empties(dtype):
    got = check("AABB", 4, 255, [0, 600, 50, 0], [10, 100, 50, 0], hq=8, hkv=2, d=128, dtype=dtype, q_pad=37, lead=3)
    assert not bool(got[:10].any()) and not bool(got[160:].any()) and bool(got[10:160].any())
    got = check("ABAB", None, None, [0, 70], [3, 70], hq=4, hkv=4, d=64, dtype=dtype, q_pad=1)
    assert not bool(got[:3].any()) and not bool(got[73:].any())
    hip = ops()[0]
    q, k, v, cu_q, cu_kv = packed_inputs([40], [40], hq=4, hkv=2, d=64, dtype=dtype)
    one = torch.zeros(1, dtype=torch.int32)
    out = on_gpu(hip, (q, k, v, one, one))                                   # batch = 0: every row is padding
    assert out.shape == q.shape and not bool(out.any())
    out = on_gpu(hip, (q[:0], k, v, one, one))                               # Tq = 0
    assert out.shape == (0, 4, 64)
    out = on_gpu(hip, (q, k[:0], v[:0], cu_q, torch.zeros(2, dtype=torch.int32)))   # Tk = 0: no key anywhere
    assert out.shape == q.shape and not bool(out.any())


def test_graph_capture_replays_with_new_lengths():
    q, k, v, cu_q, cu_kv = (x.to(DEV) for x in packed_inputs([700, 300, 90], [200, 300, 40], hq=8, hkv=2, d=128, seed=11))
    hip, ref = ops("AABB", 4, 255)
    hip.forward(q, k, v, cu_q, cu_kv)                                        # warm-up (library load, attributes)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            out = hip.forward(q, k, v, cu_q, cu_kv, max_q_len=300, max_total_seq_len=700)
    out.fill_(7.0)
    cu_q.copy_(cumulative([150, 0, 33]).to(DEV))
    cu_kv.copy_(cumulative([650, 10, 33], 2).to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    want = ref.forward(q.cpu(), k.cpu(), v.cpu(), cu_q.cpu(), cu_kv.cpu())
    assert_close_tree(to_cpu(out), want, ATOL, RTOL)
    assert not bool(out[183:].any())


def test_offsets_past_4_gib():
    """A token stride of 2^20 elements: the second sequence's rows start 4 GiB and more behind the base."""
    free, _ = torch.cuda.mem_get_info()
    if free < 8 << 30:
        pytest.skip(f"needs 8 GiB of free device memory for the 5 GiB K/V buffer, {free >> 20} MiB are free")
    hkv, d, stride, kv_tokens = 2, 128, 1 << 20, 2300
    q, k, v, cu_q, cu_kv = packed_inputs([1990, 190], [150, 190], hq=8, hkv=hkv, d=d, lead=110, tail=10, seed=13)
    assert k.shape[0] == kv_tokens and int(cu_kv[1]) == 2100
    # one buffer, K in the first 256 elements of each token's 2^20, V in the next 256; only the viewed elements are written
    buf = torch.empty((kv_tokens + 1) * stride, dtype=torch.bfloat16, device=DEV)
    assert buf.numel() * 2 > 4 << 30
    k_view = torch.as_strided(buf, (kv_tokens, hkv, d), (stride, d, 1), 0)
    v_view = torch.as_strided(buf, (kv_tokens, hkv, d), (stride, d, 1), hkv * d)
    k_view.copy_(k.to(DEV))
    v_view.copy_(v.to(DEV))
    assert (kv_tokens - 1) * stride * 2 > 4 << 30
    for glob, local in [(None, None), (4, 127)]:
        hip, ref = ops("AABB", glob, local)
        got = on_gpu(hip, (q, k_view, v_view, cu_q, cu_kv))
        assert ":fast_stage:" in expect_tag(glob, local)
        assert_close_tree(to_cpu(got), ref.forward(q, k, v, cu_q, cu_kv), ATOL, RTOL)
    del buf, k_view, v_view
    torch.cuda.empty_cache()


def test_validate_switch_raises_on_every_contract_breach(monkeypatch):
    monkeypatch.setenv("MOJO_HIP_VALIDATE", "1")
    hip = ops()[0]
    q, k, v, cu_q, cu_kv = (x.to(DEV) for x in packed_inputs([40, 30], [20, 30], hq=4, hkv=2, d=64, q_pad=2, tail=2))
    hip.forward(q, k, v, cu_q, cu_kv, max_q_len=30, max_total_seq_len=40)     # inside the contract: no error

    def cu(*vals):
        return torch.tensor(vals, dtype=torch.int32, device=DEV)

    breaches = [
        (cu(0, 30, 20), cu_kv, {}, "non-decreasing"),                       # cu_q_lens decreases
        (cu_q, cu(0, 40, 30), {}, "non-decreasing"),                        # cu_total_seq_lens decreases
        (cu(1, 20, 50), cu_kv, {}, "start at 0"),                           # cu_q_lens[0] != 0
        (cu(0, 20, 53), cu(0, 40, 72), {}, "end past"),                     # cu_q_lens[-1] > Tq
        (cu_q, cu(0, 40, 73), {}, "end past"),                              # cu_total_seq_lens[-1] > Tk
        (cu(0, 20, 50), cu(0, 40, 60), {}, "fewer keys"),                   # kv_len 20 < q_len 30
        (cu_q, cu_kv, {"max_q_len": 29}, "exceeds"),
        (cu_q, cu_kv, {"max_total_seq_len": 39}, "exceeds"),
    ]
    for cq, ckv, kw, text in breaches:
        with pytest.raises(ValueError, match=text):
            hip.forward(q, k, v, cq, ckv, **kw)
