"""GPU parity of the int8 paged KV cache ops through the C ABI; oracle = oracle/kv_int8.py on CPU.

Store: bit-exact.  Decode and prefill: atol = rtol = 2e-2 on every element (decode: the reference's own bound,
tests/accuracy/operators/test_attention_quant.py:460-461; prefill: the project's rule for GQA prefill, stricter than the
reference's 5e-2 on 90 % of the elements)."""
import math

import pytest
import torch

import oracle.kv_int8 as G
from conftest import load_golden
from hip_utils import DEV, assert_close_tree, hip_cls, last_launch, run_hip_case, switch_env, to_cpu, torch_cls
from mojo_opset_amd.core.operators.kv_cache import build_paged_kv_chunk_metadata

pytestmark = pytest.mark.gpu
ATOL = RTOL = 2e-2
DEC, PRE, STORE = "MojoPagedDecodeGQAWithKVDequant", "MojoPagedPrefillGQAWithKVDequant", "MojoStorePagedKVCacheC8"


def cu(lens):
    return torch.tensor([0] + list(torch.tensor(lens).cumsum(0).tolist()), dtype=torch.int32)


def make_inputs(hq, hkv, d, page, kv_lens, q_rows, seed=0, dtype=torch.bfloat16, spare=10):
    """Random float pools quantised with the reference's recipe (per-channel amax / 127, clamp 1e-5, bf16 scales), a
    shuffled table padded with -1."""
    g = torch.Generator().manual_seed(seed)
    need = [(n + page - 1) // page for n in kv_lens]
    total = max(sum(need), 1) + spare
    k8, ks = G.quantize_kv_cache(torch.randn(total, hkv, page, d, generator=g))
    v8, vs = G.quantize_kv_cache(torch.randn(total, hkv, page, d, generator=g))
    table = torch.full((len(kv_lens), max(max(need), 1)), -1, dtype=torch.int32)
    free = torch.randperm(total, generator=g, dtype=torch.int32)
    at = 0
    for b, n in enumerate(need):
        table[b, :n] = free[at: at + n]
        at += n
    q = torch.randn(q_rows, hq, d, generator=g).to(dtype)
    return q, k8, ks, v8, vs, table


def dev(*ts):
    return [None if t is None else t.to(DEV) for t in ts]


def run_decode(layout, q, k8, ks, v8, vs, lens, table, **kw):
    op = hip_cls(DEC)(gqa_layout=layout)
    out = op(*dev(q, None, k8, ks, v8, vs, lens, table), **kw)
    torch.cuda.synchronize()
    assert ":kv8" in last_launch() and last_launch().startswith("decode_mfma:")
    return out


def ref_decode(layout, q, k8, ks, v8, vs, lens, table):
    ref = torch_cls(DEC)(gqa_layout=layout)
    if q.dtype != torch.bfloat16:                 # (the constructor admits bf16 only; the forward's math is dtype-generic)
        ref.query_dtype = q.dtype
    return ref(q, None, k8, ks, v8, vs, lens, table)


def check(got, want, what=""):
    diff = (got.float() - want.float()).abs()
    print(f"{what}: max |diff| {float(diff.max()) if diff.numel() else 0.0:.5f}")
    assert_close_tree(got, want, ATOL, RTOL)


# ---- recorded vectors -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [pytest.param(c, id=f"store-{i}") for i, c in enumerate(load_golden("paged_kv_int8_store"))])
def test_store_vectors_bit_exact(case):
    kc, vc = to_cpu(run_hip_case(case))
    assert torch.equal(kc, case["out"][0]) and torch.equal(vc, case["out"][1])


@pytest.mark.parametrize("case", [pytest.param(c, id=f"{c['op'][9:16]}-{i}") for i, c in enumerate(
    load_golden("paged_kv_int8_decode") + load_golden("paged_kv_int8_prefill")) if c["ctor"]["kwargs"]["compute_dtype"] != torch.int8])
def test_attention_vectors(case):
    check(to_cpu(run_hip_case(case)), case["out"], case["op"])
    assert "kv8" in last_launch()


# ---- store ------------------------------------------------------------------------------------------------------------
STORE_PATTERNS = [
    (2, 2, 128, 128, [0, 0], [130, 33]), (2, 2, 128, 128, [32, 35], [1, 1]), (2, 2, 128, 128, [15, 40], [788, 126]),
    (2, 2, 128, 256, [15, 40], [788, 126]), (2, 2, 128, 512, [255, 511], [300, 257]), (2, 2, 128, 1024, [511, 1023], [600, 513]),
    (2, 2, 128, 2048, [1023, 2047], [900, 1025]), (1, 1, 128, 128, [0], [5]), (1, 1, 128, 128, [5], [1]),
    (1, 1, 128, 512, [510], [3]), (1, 1, 128, 1024, [1022], [2]), (1, 1, 128, 2048, [2046], [2]),
    (3, 2, 128, 128, [32, -1, 35], [1, 1, 1]), (3, 2, 128, 128, [0, -1, 5], [4, 0, 2]), (3, 2, 128, 512, [510, -1, 700], [4, 1, 300]),
    (3, 2, 128, 1024, [1020, -1, 1530], [8, 1, 520]), (3, 2, 128, 2048, [2040, -1, 3000], [16, 1, 900]),
    (8, 2, 128, 128, [224, 542, 34, 41, 54, 57, 65, 0], [432, 84, 977, 93, 23, 89, 31, 555]),
    (8, 2, 128, 128, [772, 974, 3232, 43, 77, 7633, 888, 1], [1] * 8),
    (8, 2, 128, 512, [224, 542, 34, 41, 54, 57, 65, 0], [432, 84, 977, 93, 23, 89, 31, 555]),
    (8, 2, 128, 1024, [900, 1500, 34, 41, 54, 57, 65, 0], [700, 600, 977, 93, 23, 89, 31, 555]),
    (8, 2, 128, 2048, [1800, 2500, 34, 41, 54, 57, 65, 0], [900, 1200, 977, 93, 23, 89, 31, 555]),
    (8, 2, 128, 512, [772, 974, 3232, 43, 77, 7633, 888, 1], [1] * 8),
    (8, 2, 128, 1024, [1023, 1024, 3232, 43, 77, 7633, 888, 1], [1] * 8),
    (8, 2, 128, 2048, [2047, 2048, 3232, 43, 77, 7633, 888, 1], [1] * 8),
]


def store_case(pattern, state_dtype, scale_dtype, seed):
    batch, heads, d, page, ctx, q_lens = pattern
    g = torch.Generator().manual_seed(seed)
    decode = all(n == 1 for n in q_lens)
    end = [max(c, 0) + n for c, n in zip(ctx, q_lens)]
    need = [max((e + page - 1) // page, 1) for e in end]
    total = sum(need) + 2
    table = torch.full((batch, max(need)), -1, dtype=torch.int32)
    free = torch.randperm(total, generator=g, dtype=torch.int32)
    at = 0
    for b, n in enumerate(need):
        table[b, :n] = free[at: at + n]
        at += n
    tokens = batch if decode else sum(q_lens)
    ks = torch.randn(tokens, heads, d, generator=g).to(state_dtype)
    vs = torch.randn(tokens, heads, d, generator=g).to(state_dtype)
    scales = torch.randn(2, heads, d, generator=g)            # both signs, as the reference test draws them
    scales = (scales.sign() * scales.abs().clamp(min=1e-3)).to(scale_dtype)
    kc = torch.randint(-128, 128, (total, heads, page, d), generator=g, dtype=torch.int8)
    vc = torch.randint(-128, 128, (total, heads, page, d), generator=g, dtype=torch.int8)
    return ks, vs, kc, vc, scales[0], scales[1], table, (None if decode else cu(q_lens)), torch.tensor(ctx, dtype=torch.int32)


@pytest.mark.parametrize("dtypes", [(torch.bfloat16, torch.bfloat16), (torch.bfloat16, torch.float32), (torch.float16, torch.float16),
                                    (torch.float16, torch.float32)], ids=["bf16_bf16", "bf16_f32", "f16_f16", "f16_f32"])
@pytest.mark.parametrize("form", ["plan", "legacy"])
def test_store_is_bit_exact_over_the_reference_patterns(dtypes, form):
    op, ref = hip_cls(STORE)(), torch_cls(STORE)()
    worst = 0
    for i, pattern in enumerate(STORE_PATTERNS):
        ks, vs, kc, vc, ksc, vsc, table, cu_q, ctx = store_case(pattern, *dtypes, seed=i)
        if form == "plan":
            plan = build_paged_kv_chunk_metadata(table, cu_q, ctx, pattern[3])
            want = ref(ks, vs, kc.clone(), vc.clone(), ksc, vsc, chunk_metadata=plan)
            got = op(*dev(ks, vs, kc, vc, ksc, vsc), chunk_metadata=plan.to(DEV))
        else:
            want = ref(ks, vs, kc.clone(), vc.clone(), ksc, vsc, table, cu_q, ctx)
            got = op(*dev(ks, vs, kc, vc, ksc, vsc, table, cu_q, ctx))
        for a, b in zip(to_cpu(got), want):
            worst = max(worst, int((a.int() - b.int()).abs().max()))
            assert torch.equal(a, b), f"pattern {i}: {int((a != b).sum())} of {a.numel()} bytes differ (max {worst})"
    print("store max |diff|:", worst)


# ---- decode -----------------------------------------------------------------------------------------------------------
DECODE_CFGS = [(8, 16, 4, 128, 1024, 32), (8, 16, 4, 96, 1024, 128), (4, 8, 1, 128, 8192, 1024), (4, 8, 1, 128, 2048, 1024),
               (4, 8, 2, 128, 2048, 128), (5, 12, 3, 64, 257, 16), (6, 24, 6, 80, 513, 64)]


@pytest.mark.parametrize("cfg", DECODE_CFGS, ids=["M_BF16", "M_BF16_PADDIM", "M_BF16_LONG", "M_BF16_BIGPAGE", "M_BF16_GROUP",
                                                  "M_BF16_VARLEN_BLK16_D64", "M_BF16_VARLEN_BLK64_D80"])
@pytest.mark.parametrize("layout", ["ABAB", "AABB"])
def test_decode_reference_space(cfg, layout):
    batch, hq, hkv, d, max_len, page = cfg
    g = torch.Generator().manual_seed(sum(cfg))
    lens = torch.randint(1, max_len + 1, (batch,), generator=g, dtype=torch.int32)
    lens[0] = max_len
    q, k8, ks, v8, vs, table = make_inputs(hq, hkv, d, page, lens.tolist(), batch, seed=sum(cfg))
    got = run_decode(layout, q, k8, ks, v8, vs, lens, table, softmax_scale=1.0 / math.sqrt(d), max_total_seq_len=max_len)
    check(to_cpu(got), ref_decode(layout, q, k8, ks, v8, vs, lens, table), f"decode {cfg} {layout}")
    again = run_decode(layout, q, k8, ks, v8, vs, lens, table)            # no hint: sized on the table's width
    check(to_cpu(again), ref_decode(layout, q, k8, ks, v8, vs, lens, table), "  no hint")


@pytest.mark.parametrize("layout", ["ABAB", "AABB"])
def test_decode_headline_geometry_ragged(layout):
    g = torch.Generator().manual_seed(7)
    lens = torch.randint(1, 4097, (8,), generator=g, dtype=torch.int32)
    lens[0], lens[1] = 4096, 2049
    q, k8, ks, v8, vs, table = make_inputs(32, 8, 128, 16, lens.tolist(), 8, seed=7)
    got = run_decode(layout, q, k8, ks, v8, vs, lens, table, max_total_seq_len=4096)
    check(to_cpu(got), ref_decode(layout, q, k8, ks, v8, vs, lens, table), "headline ragged")


@pytest.mark.parametrize("hint", [None, 600, 20000], ids=["table", "fused", "split"])
def test_decode_lengths_at_tile_chunk_and_page_boundaries(hint):
    """One short of / on / one past the 16-token sub-tile, the 32-token step, the 128-token minimum chunk and the page; with
    a 20000-token hint the rows take the split + merge form (more than 8 chunks)."""
    lens = [1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 127, 128, 129, 255, 256, 257, 511, 512, 513]
    page = 64
    q, k8, ks, v8, vs, table = make_inputs(8, 2, 128, page, lens, len(lens), seed=3)
    if hint == 20000:
        wide = torch.full((len(lens), 20000 // page + 1), -1, dtype=torch.int32)
        wide[:, : table.shape[1]] = table
        table = wide
    lens_t = torch.tensor(lens, dtype=torch.int32)
    kw = {} if hint is None else {"max_total_seq_len": hint}
    got = run_decode("AABB", q, k8, ks, v8, vs, lens_t, table, **kw)
    assert ("split+merge" in last_launch()) == (hint == 20000)
    check(to_cpu(got), ref_decode("AABB", q, k8, ks, v8, vs, lens_t, table), f"boundaries hint={hint}")


def emulate_folded_decode(layout, q, k8, ks, v8, vs, lens, table, scale):
    """CPU emulation of the kernel's folded numerics: q' = q * key_scale rounded to fp16, fp32 scores over the int8 keys,
    fp32 softmax statistics, probabilities rounded to fp16 for the second product (the row sum takes them unrounded),
    value_scale applied to the fp32 sums, one rounding to the query dtype."""
    batch, hq, d = q.shape
    hkv, page = k8.shape[1], k8.shape[2]
    group = hq // hkv
    out = torch.zeros_like(q)
    for b, n in enumerate(lens.tolist()):
        if n == 0:
            continue
        blocks = (n + page - 1) // page
        kk = k8[table[b, :blocks]].permute(1, 0, 2, 3).reshape(hkv, -1, d)[:, :n].float()
        vv = v8[table[b, :blocks]].permute(1, 0, 2, 3).reshape(hkv, -1, d)[:, :n].float()
        for h in range(hq):
            kvh = h % hkv if layout == "ABAB" else h // group
            qp = (q[b, h].float() * ks[kvh].float()).half().float()
            s_ = (kk[kvh] @ qp) * scale
            p = torch.exp(s_ - s_.max())
            o = (p.half().float() @ vv[kvh]) * vs[kvh].float() / p.sum()
            out[b, h] = o.to(q.dtype)
    return out


SHORT_LENS = [1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 127, 128, 129, 257]


@pytest.mark.parametrize("geom", [(12, 3, 64, 16), (24, 6, 80, 16), (8, 2, 96, 32), (16, 1, 128, 16), (4, 4, 128, 16), (16, 1, 64, 64),
                                  (3, 3, 80, 48), (32, 2, 96, 16)],
                         ids=["D64_g4", "D80_g4", "D96_g4", "D128_g16", "D128_g1", "D64_g16", "D80_g1_page48", "D96_g16"])
@pytest.mark.parametrize("layout", ["ABAB", "AABB"])
def test_decode_short_rows_every_head_dim_and_group(geom, layout):
    """Short rows (outputs of magnitude ~1, where the 2e-2 bound bites) at the boundary lengths, for every head_dim
    instance (zero-padded query pieces at 80 / 96; 16 / 12 / 10 / 8 V rows per load) and groups of 1, 4 and 16 heads.

    Second, tighter check against a CPU emulation of the kernel's own folded numerics.  Bound from the number formats, not
    from the kernel: each fp16 probability carries a relative error of at most 2^-12, so a row's sum of p * v is off by at
    most 2^-12 * max|v| (|v| <= 4 for these inputs: 1e-3), on either side -> atol 2e-3; the fp32 sums differ only by their
    order; the final rounding of two such values to bf16 can land on neighbouring numbers -> rtol 2^-7 (one bf16 ulp)."""
    hq, hkv, d, page = geom
    q, k8, ks, v8, vs, table = make_inputs(hq, hkv, d, page, SHORT_LENS, len(SHORT_LENS), seed=sum(geom))
    lens = torch.tensor(SHORT_LENS, dtype=torch.int32)
    got = to_cpu(run_decode(layout, q, k8, ks, v8, vs, lens, table))
    check(got, ref_decode(layout, q, k8, ks, v8, vs, lens, table), f"short rows {geom} {layout}")
    emu = emulate_folded_decode(layout, q, k8, ks, v8, vs, lens, table, 1.0 / math.sqrt(d))
    print(f"  vs emulation: max |diff| {float((got.float() - emu.float()).abs().max()):.5f}")
    assert_close_tree(got, emu, 2e-3, 2.0 ** -7)


def test_decode_zero_length_rows_fp16_and_truncation():
    lens = [0, 5, 0, 300, 1, 0]
    q, k8, ks, v8, vs, table = make_inputs(8, 2, 128, 16, lens, len(lens), seed=5, dtype=torch.float16)
    lens_t = torch.tensor(lens, dtype=torch.int32)
    out = to_cpu(run_decode("AABB", q, k8, ks, v8, vs, lens_t, table))
    assert out.dtype == torch.float16 and torch.count_nonzero(out[[0, 2, 5]]) == 0
    check(out, ref_decode("AABB", q, k8, ks, v8, vs, lens_t, table), "fp16 + zero rows")
    # a hint below a device length truncates that row to the hint (as the 16-bit op)
    cut = to_cpu(run_decode("AABB", q, k8, ks, v8, vs, lens_t, table, max_total_seq_len=128))
    short = torch.tensor([0, 5, 0, 128, 1, 0], dtype=torch.int32)
    check(cut, ref_decode("AABB", q, k8, ks, v8, vs, short, table), "truncated")


@pytest.mark.parametrize("layout", ["ABAB", "AABB"])
def test_decode_padded_rows_under_graph_replay(layout):
    """Static buffers mutated between replays; padded rows (seq_len = 0, table -1) are LEFT UNCHANGED by a replay and are
    zeros eagerly — the `leave_empty_rows` contract of the 16-bit op."""
    B, hq, hkv, d, page, max_len = 8, 16, 4, 128, 32, 1024
    width = max_len // page
    pool = B * width + 10

    def fresh(cur_b, seed):
        g = torch.Generator().manual_seed(seed)
        lens = torch.randint(1, max_len + 1, (cur_b,), generator=g, dtype=torch.int32)
        q, k8, ks, v8, vs, table = make_inputs(hq, hkv, d, page, lens.tolist(), cur_b, seed=seed, spare=0)
        return q, k8, ks, v8, vs, lens, table

    q, k8, ks, v8, vs, lens, table = fresh(B, 11)
    sq = q.to(DEV)
    sk, sv = torch.zeros(pool, hkv, page, d, dtype=torch.int8, device=DEV), torch.zeros(pool, hkv, page, d, dtype=torch.int8, device=DEV)
    sks, svs = ks.to(DEV), vs.to(DEV)
    sl = lens.to(DEV)
    st = torch.full((B, width), -1, dtype=torch.int32, device=DEV)
    sk[: k8.shape[0]], sv[: v8.shape[0]] = k8.to(DEV), v8.to(DEV)
    st[:, : table.shape[1]] = table.to(DEV)
    op = hip_cls(DEC)(gqa_layout=layout)
    op(sq, None, sk, sks, sv, svs, sl, st, max_total_seq_len=max_len)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = op(sq, None, sk, sks, sv, svs, sl, st, max_total_seq_len=max_len)
    graph.replay()
    torch.cuda.synchronize()
    check(to_cpu(out), ref_decode(layout, q, k8, ks, v8, vs, lens, table), "replay 0")
    for step in range(3):
        cur_b = 2 + 2 * step
        cq, ck, cks, cv, cvs, cl, ct = fresh(cur_b, 100 + step)
        sk[: ck.shape[0]].copy_(ck.to(DEV))
        sv[: cv.shape[0]].copy_(cv.to(DEV))
        sks.copy_(cks.to(DEV))
        svs.copy_(cvs.to(DEV))
        sq[:cur_b].copy_(cq.to(DEV))
        sl[:cur_b].copy_(cl.to(DEV))
        sl[cur_b:] = 0
        st.fill_(-1)
        st[:cur_b, : ct.shape[1]].copy_(ct.to(DEV))
        keep = out[cur_b:].clone()
        graph.replay()
        torch.cuda.synchronize()
        check(to_cpu(out[:cur_b]), ref_decode(layout, cq, ck, cks, cv, cvs, cl, ct), f"replay {step + 1}")
        assert torch.equal(out[cur_b:], keep), "padded rows were modified by the replay"
        eager = op(sq, None, sk, sks, sv, svs, sl, st, max_total_seq_len=max_len)
        assert torch.count_nonzero(eager[cur_b:]) == 0
        assert torch.equal(eager[:cur_b], out[:cur_b])
        forced = op(sq, None, sk, sks, sv, svs, sl, st, max_total_seq_len=max_len, leave_empty_rows=True)
        assert torch.equal(forced[:cur_b], out[:cur_b])


def test_store_then_decode_round_trip():
    """hip store into a zeroed int8 cache, then hip decode over it == hip decode over the golden-quantised cache, bit for bit."""
    hq, hkv, d, page, lens = 8, 2, 128, 16, [70, 33, 129]
    g = torch.Generator().manual_seed(9)
    need = [(n + page - 1) // page for n in lens]
    total = sum(need) + 2
    table = torch.full((len(lens), max(need)), -1, dtype=torch.int32)
    free = torch.randperm(total, generator=g, dtype=torch.int32)
    at = 0
    for b, n in enumerate(need):
        table[b, :n] = free[at: at + n]
        at += n
    ks_ = torch.randn(sum(lens), hkv, d, generator=g).to(torch.bfloat16)
    vs_ = torch.randn(sum(lens), hkv, d, generator=g).to(torch.bfloat16)
    kscale = (ks_.float().abs().amax(dim=0) / 127).clamp(min=1e-5).to(torch.bfloat16)
    vscale = (vs_.float().abs().amax(dim=0) / 127).clamp(min=1e-5).to(torch.bfloat16)
    ctx = torch.zeros(len(lens), dtype=torch.int32)
    zeros = lambda: torch.zeros(total, hkv, page, d, dtype=torch.int8)  # noqa: E731
    kc_ref, vc_ref = torch_cls(STORE)()(ks_, vs_, zeros(), zeros(), kscale, vscale, table, cu(lens), ctx)
    kc, vc = hip_cls(STORE)()(*dev(ks_, vs_, zeros(), zeros(), kscale, vscale, table, cu(lens), ctx))
    assert torch.equal(to_cpu(kc), kc_ref) and torch.equal(to_cpu(vc), vc_ref)
    q = torch.randn(len(lens), hq, d, generator=g).to(torch.bfloat16)
    lens_t = torch.tensor(lens, dtype=torch.int32)
    op = hip_cls(DEC)()
    a = op(q.to(DEV), None, kc, kscale.to(DEV), vc, vscale.to(DEV), lens_t.to(DEV), table.to(DEV))
    b = op(*dev(q, None, kc_ref, kscale, vc_ref, vscale, lens_t, table))
    assert torch.equal(a, b)
    check(to_cpu(a), ref_decode("AABB", q, kc_ref, kscale, vc_ref, vscale, lens_t, table), "round trip")


# ---- prefill ----------------------------------------------------------------------------------------------------------
# (batch, hq, hkv, d, max q_len, max cached, page): the reference's list inside the envelope (groups 1/2/4/8, head_dim 64/96/128):
# all 14 of its 16 configs but the head_dim 192 and head_dim 80 ones
PREFILL_CFGS = [(2, 16, 4, 128, 1024, 0, 32), (2, 16, 4, 96, 1024, 0, 128), (2, 8, 1, 128, 512, 1024, 128), (2, 8, 1, 128, 1024, 2048, 1024),
                (2, 8, 2, 128, 1024, 0, 128), (3, 12, 3, 64, 257, 513, 16), (1, 16, 4, 128, 128, 0, 16), (2, 24, 6, 128, 255, 129, 32),
                (3, 16, 4, 128, 513, 257, 64), (4, 24, 6, 128, 769, 511, 128), (5, 16, 4, 128, 1025, 333, 256),
                (6, 24, 6, 128, 1537, 777, 128), (5, 16, 4, 128, 2049, 1025, 256), (4, 24, 6, 128, 3073, 1537, 256)]


def run_prefill(layout, q, k8, ks, v8, vs, q_lens, kv_lens, table, **kw):
    op = hip_cls(PRE)(gqa_layout=layout)
    out = op(*dev(q, None, k8, ks, v8, vs, cu(q_lens), table), cu_total_seq_lens=cu(kv_lens).to(DEV), **kw)
    torch.cuda.synchronize()
    assert "kv8" in last_launch()
    want = torch_cls(PRE)(gqa_layout=layout)(q, None, k8, ks, v8, vs, cu(q_lens), table, cu_total_seq_lens=cu(kv_lens))
    return to_cpu(out), want


@pytest.mark.parametrize("cfg", PREFILL_CFGS, ids=[f"B{c[0]}_H{c[1]}_{c[2]}_D{c[3]}_q{c[4]}_c{c[5]}_p{c[6]}" for c in PREFILL_CFGS])
@pytest.mark.parametrize("layout", ["ABAB", "AABB"])
def test_prefill_reference_space(cfg, layout):
    batch, hq, hkv, d, max_q, max_cached, page = cfg
    g = torch.Generator().manual_seed(sum(cfg))
    q_lens = torch.randint(1, max_q + 1, (batch,), generator=g).tolist()
    q_lens[0] = max_q
    cached = torch.randint(0, max_cached + 1, (batch,), generator=g).tolist() if max_cached else [0] * batch
    kv_lens = [a + c for a, c in zip(q_lens, cached)]
    q, k8, ks, v8, vs, table = make_inputs(hq, hkv, d, page, kv_lens, sum(q_lens), seed=sum(cfg))
    got, want = run_prefill(layout, q, k8, ks, v8, vs, q_lens, kv_lens, table, max_q_len=max(q_lens), max_total_seq_len=max(kv_lens))
    check(got, want, f"prefill {cfg} {layout}")


def test_prefill_ragged_with_an_empty_sequence_and_no_hints():
    q_lens, kv_lens = [70, 0, 33, 200], [300, 0, 33, 200]
    q, k8, ks, v8, vs, table = make_inputs(8, 2, 128, 16, kv_lens, sum(q_lens), seed=21)
    got, want = run_prefill("AABB", q, k8, ks, v8, vs, q_lens, kv_lens, table)
    check(got, want, "prefill ragged")


def test_prefill_table_with_valid_ids_past_a_rows_length():
    """Table columns past a row's length name real pages (a pre-allocated cache), here filled with 127s: they are neither
    gathered nor read, so the result is that of the -1 padded table."""
    q_lens, kv_lens = [40, 17], [130, 17]
    q, k8, ks, v8, vs, table = make_inputs(8, 2, 128, 16, kv_lens, sum(q_lens), seed=23, spare=4)
    want = torch_cls(PRE)()(q, None, k8, ks, v8, vs, cu(q_lens), table, cu_total_seq_lens=cu(kv_lens))
    spare = [i for i in range(k8.shape[0]) if i not in set(table[table >= 0].tolist())]
    k8[spare], v8[spare] = 127, 127
    full = table.clone()
    full[full < 0] = spare[0]
    op = hip_cls(PRE)()
    for hint in (None, 130, 160):
        got = op(*dev(q, None, k8, ks, v8, vs, cu(q_lens), full), cu_total_seq_lens=cu(kv_lens).to(DEV), max_total_seq_len=hint)
        check(to_cpu(got), want, f"prefill full table hint={hint}")


def test_prefill_hint_below_a_length_is_refused_under_validate():
    """`max_total_seq_len` sizes the scratch pages, so it must be an upper bound; MOJO_HIP_VALIDATE=1 checks it."""
    q_lens, kv_lens = [40, 17], [130, 17]
    q, k8, ks, v8, vs, table = make_inputs(8, 2, 128, 16, kv_lens, sum(q_lens), seed=24)
    args = dev(q, None, k8, ks, v8, vs, cu(q_lens), table)
    with switch_env(MOJO_HIP_VALIDATE="1"):
        with pytest.raises(ValueError):
            hip_cls(PRE)()(*args, cu_total_seq_lens=cu(kv_lens).to(DEV), max_total_seq_len=128)
        hip_cls(PRE)()(*args, cu_total_seq_lens=cu(kv_lens).to(DEV), max_total_seq_len=130)


def test_decode_query_operand_saturates_instead_of_overflowing():
    """q * key_scale lives in fp16: a product beyond 65504 saturates (finite output), it does not become inf / NaN."""
    lens = [40]
    q, k8, ks, v8, vs, table = make_inputs(4, 1, 64, 16, lens, 1, seed=25)
    q[0, 0, 0] = 3.0e4
    ks[0, 0] = 8.0
    out = to_cpu(run_decode("AABB", q, k8, ks, v8, vs, torch.tensor(lens, dtype=torch.int32), table))
    assert bool(torch.isfinite(out.float()).all())


# ---- decode edges: holes, unused table entries, relabelled pages, the cached instance -------------------------------------
HOLE_LENS = [700, 129, 40]                         # row 0: 44 pages of 16 tokens
LONG_HOLE_LENS = [4200, 40]                        # row 0: 263 pages — the hole scan's second batch of 256 pages runs


def chunk_first_pages(n, page=16):
    """First page of the second chunk of an n-token row for every chunk count a fused launch may choose (2 .. 8 waves): equal
    pieces of whole 16-token tiles, 128 tokens at least (the rule `test_decode_lengths_at_tile_chunk_and_page_boundaries` names)."""
    return sorted({-(-max(-(-n // c), 128) // 16) * 16 // page for c in range(2, 9)})


HOLES = {"first": (HOLE_LENS, [0]), "mid": (HOLE_LENS, [20]), "chunk_first": (HOLE_LENS, chunk_first_pages(HOLE_LENS[0])),
         "row_last": (HOLE_LENS, [43]), "page_258": (LONG_HOLE_LENS, [258])}


def hole_case(lens, seed=41):
    hq, hkv = (4, 1) if lens is LONG_HOLE_LENS else (8, 2)
    q, k8, ks, v8, vs, table = make_inputs(hq, hkv, 128, 16, lens, len(lens), seed=seed)
    spare = [i for i in range(k8.shape[0]) if i not in set(table[table >= 0].tolist())]
    k8[spare[0]], v8[spare[0]] = 0, 0              # the oracle's page of zero K and V
    k8[spare[1]], v8[spare[1]] = 127, 127          # what an unused table entry may name
    return q, k8, ks, v8, vs, table, spare[0], spare[1]


def holed(table, page_idx, zero_page):
    """(the table with -1 at row 0's page ``page_idx``, the oracle's copy: that entry and every later one of the row name the
    page of zeros — pages at and behind the first negative id read as zero K/V, csrc/paged_decode_kv8.h)."""
    hole, filled = table.clone(), table.clone()
    hole[0, page_idx] = -1
    filled[0, page_idx:] = zero_page
    return hole, filled


@pytest.mark.parametrize("where", list(HOLES))
@pytest.mark.parametrize("form", ["fused", "split"])
@pytest.mark.parametrize("layout", ["ABAB", "AABB"])
def test_decode_holes_read_as_zero_keys_and_values(layout, form, where):
    lens, pages = HOLES[where]
    q, k8, ks, v8, vs, table, zero_page, _ = hole_case(lens)
    lens_t = torch.tensor(lens, dtype=torch.int32)
    assert (lens[0] + 15) // 16 > max(pages) and (where != "page_258" or pages[0] >= 256)
    # (a few rows of 4 200 tokens are planned as 33 chunks of 128 tokens, the split form: chunks of 1 024 keep them in one
    # workgroup of five waves, whose last wave scans 263 table entries)
    chunk = "1024" if (form, where) == ("fused", "page_258") else None
    with switch_env(MOJO_HIP_DECODE_FUSE="0" if form == "split" else None, MOJO_HIP_DECODE_CHUNK=chunk):
        for p in pages:
            hole, filled = holed(table, p, zero_page)
            got = to_cpu(run_decode(layout, q, k8, ks, v8, vs, lens_t, hole))
            assert ("split+merge" if form == "split" else ":fused:") in last_launch(), last_launch()
            check(got, ref_decode(layout, q, k8, ks, v8, vs, lens_t, filled), f"hole {where} page {p} {form} {layout}")
            # the same bits as the kernel's own result on the oracle's table: a hole is exactly a page of zeros
            assert torch.equal(got, to_cpu(run_decode(layout, q, k8, ks, v8, vs, lens_t, filled)))


@pytest.mark.parametrize("where", list(HOLES))
@pytest.mark.parametrize("layout", ["ABAB", "AABB"])
def test_prefill_holes_read_as_zero_keys_and_values(layout, where):
    lens, pages = HOLES[where]
    _, k8, ks, v8, vs, table, zero_page, _ = hole_case(lens)
    q_lens = [min(n, 24) for n in lens]
    hq = 4 if lens is LONG_HOLE_LENS else 8
    q = torch.randn(sum(q_lens), hq, 128, generator=torch.Generator().manual_seed(43)).to(torch.bfloat16)
    op, ref = hip_cls(PRE)(gqa_layout=layout), torch_cls(PRE)(gqa_layout=layout)
    from mojo_opset_amd.backends.hip import lib as L
    ws_bytes = max(L.load().mojo_hip_paged_prefill_gqa_kv8_workspace_bytes(q.shape[0], len(lens), hq, k8.shape[1], 128, 16, table.shape[1], 0, 0), 256)
    for p in pages:
        hole, filled = holed(table, p, zero_page)
        # the op's workspace (scratch pages included) is uninitialised memory: hand the allocator a block of NaN patterns of
        # its size to reuse, so that a scratch page that is addressed without having been gathered shows
        junk = torch.full((ws_bytes,), 0xFF, dtype=torch.uint8, device=DEV)
        del junk
        got = op(*dev(q, None, k8, ks, v8, vs, cu(q_lens), hole), cu_total_seq_lens=cu(lens).to(DEV))
        torch.cuda.synchronize()
        assert "kv8" in last_launch()
        check(to_cpu(got), ref(q, None, k8, ks, v8, vs, cu(q_lens), filled, cu_total_seq_lens=cu(lens)), f"prefill hole {where} page {p} {layout}")


@pytest.mark.parametrize("form", ["fused", "split"])
def test_decode_table_with_valid_ids_past_a_rows_length(form):
    """Table columns past a row's pages name a real page of 127s (a pre-allocated cache): never read, not one bit changes."""
    q, k8, ks, v8, vs, table, _, sevens = hole_case(HOLE_LENS)
    lens_t = torch.tensor(HOLE_LENS, dtype=torch.int32)
    wide = torch.full((table.shape[0], table.shape[1] + 5), -1, dtype=torch.int32)
    wide[:, : table.shape[1]] = table
    full = wide.clone()
    full[full < 0] = sevens
    with switch_env(MOJO_HIP_DECODE_FUSE="0" if form == "split" else None):
        for hint in (None, 700, 704):
            kw = {} if hint is None else {"max_total_seq_len": hint}
            a = run_decode("AABB", q, k8, ks, v8, vs, lens_t, wide, **kw)
            b = run_decode("AABB", q, k8, ks, v8, vs, lens_t, full, **kw)
            assert torch.equal(a, b), hint
        check(to_cpu(b), ref_decode("AABB", q, k8, ks, v8, vs, lens_t, table), f"full table {form}")


@pytest.mark.parametrize("form", ["fused", "split"])
def test_decode_relabelled_pages_and_a_second_launch_change_no_bit(form):
    from test_hip_decode_ring import relabel
    q, k8, ks, v8, vs, table, _, _ = hole_case(LONG_HOLE_LENS)
    lens_t = torch.tensor(LONG_HOLE_LENS, dtype=torch.int32)
    k2, v2, table2 = relabel(k8, v8, table)
    with switch_env(MOJO_HIP_DECODE_FUSE="0" if form == "split" else None):
        a = run_decode("AABB", q, k8, ks, v8, vs, lens_t, table)
        assert torch.equal(run_decode("AABB", q, k8, ks, v8, vs, lens_t, table), a)
        assert torch.equal(run_decode("AABB", q, k2, ks, v2, vs, lens_t, table2), a)
    check(to_cpu(a), ref_decode("AABB", q, k8, ks, v8, vs, lens_t, table), f"relabel {form}")


@pytest.mark.parametrize("form", ["fused", "split"])
@pytest.mark.parametrize("scale_dtype", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "fp16", "fp32"])
def test_decode_cached_instance_gives_the_bits_of_the_streaming_one(scale_dtype, form):
    """`MOJO_HIP_STREAM_NT=0` launches the instance with plain (cached) loads: `:cached:` in its name, the same bits."""
    q, k8, ks, v8, vs, table = make_inputs(12, 3, 96, 32, SHORT_LENS, len(SHORT_LENS), seed=47)
    ks, vs = ks.to(scale_dtype), vs.to(scale_dtype)
    lens_t = torch.tensor(SHORT_LENS, dtype=torch.int32)
    with switch_env(MOJO_HIP_DECODE_FUSE="0" if form == "split" else None):
        a = run_decode("AABB", q, k8, ks, v8, vs, lens_t, table)
        assert ":nt:" in last_launch(), last_launch()
        with switch_env(MOJO_HIP_STREAM_NT="0"):
            b = run_decode("AABB", q, k8, ks, v8, vs, lens_t, table)
            assert ":cached:" in last_launch(), last_launch()
    assert torch.equal(a, b)
    check(to_cpu(a), ref_decode("AABB", q, k8, ks, v8, vs, lens_t, table), f"cached {form} {scale_dtype}")
