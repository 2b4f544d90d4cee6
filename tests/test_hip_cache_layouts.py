"""Every paged-cache op on the cache and block-table layouts it accepts (tests/cache_layouts.py): a token-major cache seen
through a permuted view, K and V as the halves of one pool, a cache with padded rows and a block offset, an MLA cache with
``c_kv | k_pe`` in one row, and a block table that is a column slice of a wider one.

Each case is built once on the CPU (one oracle result for every layout: tests/test_cache_layouts.py shows that the goldens
return the same bits on views).  Per op, layout and launch form:
  (a) the HIP result on the strided views is within the op's own bound of the oracle (atol = rtol = 2e-2 for GQA / SWA /
      int8-KV, `check_mla` for MLA, bit equality for the stores);
  (b) it is bit-identical to the same op on `.contiguous()` copies with a dense table — a layout changes addresses, never
      arithmetic (both launch forms are printed when they differ);
  (c) `last_launch()` shows the form the case is about;
  (d) it is finite: everything a view does not cover is poison (NaN / int8 127), and so is the page every hidden table
      column names;
  (e) stores: the WHOLE storage, padding included, equals the oracle's result on a CPU clone of it.
No id outside the pool is written anywhere, and a kernel that ignored a stride would still stay inside the storage (the
dense strides are never larger than a layout's).
"""
import functools

import pytest
import torch

import cache_layouts as CL
import oracle.swa
from conftest import bit_equal
from hip_utils import DEV, assert_close_tree, hip_cls, last_launch, launches_of, switch_env, to_cpu, torch_cls
from mojo_opset_amd.core.operators.kv_cache import build_paged_kv_chunk_metadata
from test_hip_decode_gqa import make_decode_inputs
from test_hip_decode_ring import HANDOVER_LENS, paired_lens
from test_hip_kv_int8 import SHORT_LENS, STORE_PATTERNS, make_inputs as make_kv8_inputs, store_case as c8_store_case
from test_hip_mla import build as build_mla, check_mla, cu, exact_mla, make_mla, prefill_route
from test_hip_prefill_gqa import make_prefill_inputs
from test_hip_store_mla import _scenario as mla_store_scenario
from test_hip_streaming import _store_case

pytestmark = pytest.mark.gpu
ATOL = RTOL = 2e-2
# (cache layout, table layout): every cache layout once, each table slice twice; `hnd-wide` isolates the table stride
LAYOUTS = [("nhd", "offset"), ("kv_pool", "wide"), ("padded", "offset"), ("hnd", "wide")]
LAYOUT_IDS = ["-".join(p) for p in LAYOUTS]
MLA_LAYOUTS = [("fused_row", "wide"), ("fused_row", "offset"), ("dense", "offset")]
MLA_LAYOUT_IDS = ["-".join(p) for p in MLA_LAYOUTS]
BASE_LENS = (1, 17, 0, 129, 401)


def poisoned_spare(caches, table):
    """Poison one page of the pool that the table does not name; its id goes into every hidden table column."""
    return CL.poison_page(caches, CL.spare_pages(caches[0].shape[0], table)[0])


def on_views_and_dense(call, caches, table):
    """``call(*cache views, table view)`` on the strided views, then on dense copies -> (got, dense, the two launch forms)."""
    (t,) = table.views
    assert not all(c.is_contiguous() for c in caches.views) or t.stride(0) != t.shape[1]
    got = call(*caches.views, t)
    torch.cuda.synchronize()
    form = last_launch()
    dense = call(*[c.contiguous() for c in caches.views], t.contiguous())
    torch.cuda.synchronize()
    form_dense = last_launch()
    if form != form_dense:
        print(f"launch forms differ: strided {form} / dense {form_dense}")
    return got, dense, (form, form_dense)


def check_attention(call, want, caches, table, form):
    """(a) - (d) for an attention op whose bound is atol = rtol = 2e-2."""
    got, dense, forms = on_views_and_dense(call, caches, table)
    assert forms[0].startswith(form[0]) and form[1] in forms[0], (forms, form)                        # (c)
    out = to_cpu(got)
    assert bool(torch.isfinite(out.float()).all()), "poison was read"                                  # (d)
    assert_close_tree(out, want, ATOL, RTOL)                                                           # (a)
    assert torch.equal(got, dense), forms                                                              # (b)
    return out


def lay_kv(k, v, table, hidden, layout):
    return CL.lay_out_kv(k, v, layout[0]).to(DEV), CL.lay_out_table(table, layout[1], hidden).to(DEV)


# ---- 16-bit decode ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def decode_case(hq, hkv, d, page, lens, dtype=torch.bfloat16):
    q, k, v, lens_t, table = make_decode_inputs(len(lens), hq, hkv, d, 0, page, dtype=dtype, lens=list(lens), seed=hq + d + page)
    hidden = poisoned_spare([k, v], table)
    return (q, k, v, lens_t, table, hidden), torch_cls("MojoPagedDecodeGQA")()(q, k, v, lens_t, table)


DECODE_FORMS = {
    # name: (switches, (hq, hkv, d, page, lens[, dtype]), max_total_seq_len, (form prefix, form infix))
    **{f"valu_d{d}_p{p}": ({"MOJO_HIP_DECODE_MFMA": "0"}, (8, 2, d, p, BASE_LENS), None, ("decode_valu:", ""))
       for d in (128, 64) for p in (16, 64)},
    **{f"fused_d{d}_p{p}": ({"MOJO_HIP_DECODE_PAIR": "0"}, (8, 2, d, p, BASE_LENS), None, ("decode_mfma:fused", ""))
       for d in (128, 64) for p in (16, 64)},
    "paired": ({}, (32, 8, 128, 16, tuple(paired_lens("ragged"))), 600, ("decode_mfma:paired", "")),
    "grouped": ({}, (64, 8, 128, 16, (100, 700, 5000)), 5000, ("decode_mfma:grouped+merge", "")),
    "split": ({"MOJO_HIP_DECODE_FUSE": "0"}, (8, 2, 128, 16, BASE_LENS), None, ("decode_mfma:split+merge", "")),
    "long_chunks": ({"MOJO_HIP_DECODE_CHUNK": "2048"}, (4, 1, 128, 16, tuple(HANDOVER_LENS)), None, ("decode_mfma:fused", "")),
    "fp16": ({}, (8, 2, 128, 16, BASE_LENS, torch.float16), None, ("decode_mfma:", "")),
}


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("name", list(DECODE_FORMS))
def test_decode_gqa(name, layout):
    env, shape, hint, form = DECODE_FORMS[name]
    (q, k, v, lens, table, hidden), want = decode_case(*shape)
    caches, tb = lay_kv(k, v, table, hidden, layout)
    op, qd, ld = hip_cls("MojoPagedDecodeGQA")(), q.to(DEV), lens.to(DEV)
    kw = {} if hint is None else {"max_total_seq_len": hint}
    with switch_env(**env):
        out = check_attention(lambda kc, vc, t: op(qd, kc, vc, ld, t, **kw), want, caches, tb, form)
    assert torch.count_nonzero(out[lens == 0]) == 0


@functools.lru_cache(maxsize=None)
def swa_decode_case(lens, glob, local):
    q, k, v, lens_t, table = make_decode_inputs(len(lens), 8, 2, 128, 0, 16, lens=list(lens), seed=31)
    hidden = poisoned_spare([k, v], table)
    kw = dict(gqa_layout="AABB", global_window_size=glob, local_window_size=local)
    return (q, k, v, lens_t, table, hidden), oracle.swa.TorchPagedDecodeSWA(**kw).forward(q, k, v, lens_t, table), kw


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("lens", [(3000, 600, 100), (520, 17, 40)], ids=["gap", "collapsed"])
def test_decode_swa(lens, layout):
    (q, k, v, lens_t, table, hidden), want, kw = swa_decode_case(lens, 40, 500)
    caches, tb = lay_kv(k, v, table, hidden, layout)
    op, qd, ld = hip_cls("MojoPagedDecodeSWA")(**kw), q.to(DEV), lens_t.to(DEV)
    check_attention(lambda kc, vc, t: op(qd, kc, vc, ld, t), want, caches, tb, ("decode_mfma:", ":swa"))


def test_decode_host_copies_of_a_sliced_query_and_strided_lengths():
    """The query is a slice of a wider tensor and `total_seq_lens` every second element of a longer one: the host copies
    both, next to a strided cache and table that it must not copy."""
    (q, k, v, lens, table, hidden), want = decode_case(8, 2, 128, 16, BASE_LENS)
    caches, tb = lay_kv(k, v, table, hidden, ("padded", "offset"))
    q_wide = torch.full((q.shape[0], q.shape[1], 2 * q.shape[2]), float("nan"), dtype=q.dtype)
    q_wide[..., : q.shape[2]] = q
    lens_wide = torch.full((2 * lens.numel(),), 10 ** 6, dtype=torch.int32)
    lens_wide[::2] = lens
    qd, ld = q_wide.to(DEV)[..., : q.shape[2]], lens_wide.to(DEV)[::2]
    assert not qd.is_contiguous() and not ld.is_contiguous()
    op = hip_cls("MojoPagedDecodeGQA")()
    check_attention(lambda kc, vc, t: op(qd, kc, vc, ld, t), want, caches, tb, ("decode_mfma:", ""))


# ---- 16-bit prefill ---------------------------------------------------------------------------------------------------
Q_LENS, CACHED = (40, 17, 300), (90, 0, 600)
SWA_SHORT, SWA_LONG = (4, 255), (4, 1023)              # (global, local); the long one keeps a four-way key split worthwhile


def swa_kw(windows):
    return dict(gqa_layout="AABB", global_window_size=windows[0], local_window_size=windows[1])


@functools.lru_cache(maxsize=None)
def prefill_case(group, d, page, q_lens=Q_LENS, cached=CACHED, swa=None):
    hkv = 2
    q, k, v, cu_q, table, cu_kv, _ = make_prefill_inputs(list(q_lens), list(cached), hkv * group, hkv, d, page, seed=group + d + page)
    hidden = poisoned_spare([k, v], table)
    ref = oracle.swa.TorchPagedPrefillSWA(**swa_kw(swa)).forward if swa else torch_cls("MojoPagedPrefillGQA")()
    return (q, k, v, cu_q, table, cu_kv, hidden), ref(q, k, v, cu_q, table, cu_total_seq_lens=cu_kv)


PREFILL_SHAPES = {"g1_d128_p16": (1, 128, 16), "g4_d64_p128": (4, 64, 128), "g4_d128_p16": (4, 128, 16), "g1_d64_p128": (1, 64, 128)}


def run_prefill(shape, layout, swa, form, env={}):
    (q, k, v, cu_q, table, cu_kv, hidden), want = prefill_case(*shape, swa=swa)
    caches, tb = lay_kv(k, v, table, hidden, layout)
    op = hip_cls("MojoPagedPrefillSWA")(**swa_kw(swa)) if swa else hip_cls("MojoPagedPrefillGQA")()
    qd, cq, ck = q.to(DEV), cu_q.to(DEV), cu_kv.to(DEV)
    with switch_env(**env):
        check_attention(lambda kc, vc, t: op(qd, kc, vc, cq, t, cu_total_seq_lens=ck), want, caches, tb, form)


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("shape", list(PREFILL_SHAPES))
def test_prefill_gqa(shape, layout):
    run_prefill(PREFILL_SHAPES[shape], layout, None, ("prefill:", ""))


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("shape", ["g1_d128_p16", "g4_d64_p128"])
def test_prefill_swa(shape, layout):
    run_prefill(PREFILL_SHAPES[shape], layout, SWA_SHORT, ("prefill:", ":swa"))


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("swa", [None, SWA_LONG], ids=["gqa", "swa"])
def test_prefill_key_split(swa, layout):
    """One 128-query row against 6 000 keys, cut four ways along the keys (fp32 partials and a merge launch)."""
    run_prefill((4, 128, 16, (128,), (6000 - 128,)), layout, swa, ("prefill:", ":ksplit4"), env={"MOJO_HIP_PREFILL_KSPLIT": "4"})


# ---- int8 KV ----------------------------------------------------------------------------------------------------------
DEC8, PRE8 = "MojoPagedDecodeGQAWithKVDequant", "MojoPagedPrefillGQAWithKVDequant"
KV8_GEOMS = {"d64_bf16": ((12, 3, 64, 16), torch.bfloat16), "d80_fp16": ((24, 6, 80, 16), torch.float16),
             "d96_fp32": ((8, 2, 96, 32), torch.float32), "d128_fp16": ((16, 1, 128, 16), torch.float16),
             "d128_fp32": ((4, 4, 128, 16), torch.float32)}
KV8_Q_LENS = [min(n, 20) for n in SHORT_LENS]


@functools.lru_cache(maxsize=None)
def kv8_case(name, prefill):
    (hq, hkv, d, page), scale_dtype = KV8_GEOMS[name]
    q, k8, ks, v8, vs, table = make_kv8_inputs(hq, hkv, d, page, SHORT_LENS, sum(KV8_Q_LENS) if prefill else len(SHORT_LENS), seed=hq + d)
    ks, vs = ks.to(scale_dtype), vs.to(scale_dtype)
    hidden = poisoned_spare([k8, v8], table)
    if prefill:
        want = torch_cls(PRE8)()(q, None, k8, ks, v8, vs, cu(KV8_Q_LENS), table, cu_total_seq_lens=cu(SHORT_LENS))
    else:
        want = torch_cls(DEC8)()(q, None, k8, ks, v8, vs, torch.tensor(SHORT_LENS, dtype=torch.int32), table)
    return (q, k8, ks, v8, vs, table, hidden), want


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("form", ["fused", "split"])
@pytest.mark.parametrize("name", list(KV8_GEOMS))
def test_decode_kv_int8(name, form, layout):
    (q, k8, ks, v8, vs, table, hidden), want = kv8_case(name, False)
    caches, tb = lay_kv(k8, v8, table, hidden, layout)
    op = hip_cls(DEC8)()
    qd, ksd, vsd, ld = q.to(DEV), ks.to(DEV), vs.to(DEV), torch.tensor(SHORT_LENS, dtype=torch.int32, device=DEV)
    with switch_env(**({"MOJO_HIP_DECODE_FUSE": "0"} if form == "split" else {})):
        check_attention(lambda kc, vc, t: op(qd, None, kc, ksd, vc, vsd, ld, t), want, caches, tb,
                        ("decode_mfma:" + ("fused" if form == "fused" else "split+merge"), ":kv8"))


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("name", ["d64_bf16", "d96_fp32", "d128_fp32"])
def test_prefill_kv_int8(name, layout):
    (q, k8, ks, v8, vs, table, hidden), want = kv8_case(name, True)
    caches, tb = lay_kv(k8, v8, table, hidden, layout)
    op = hip_cls(PRE8)()
    qd, ksd, vsd, cq, ck = q.to(DEV), ks.to(DEV), vs.to(DEV), cu(KV8_Q_LENS).to(DEV), cu(SHORT_LENS).to(DEV)
    check_attention(lambda kc, vc, t: op(qd, None, kc, ksd, vc, vsd, cq, t, cu_total_seq_lens=ck), want, caches, tb, ("", "kv8"))


# ---- MLA --------------------------------------------------------------------------------------------------------------
MLA_GEOMS = {"r512": (16, 128, 64, 128, 512, 0.05), "r32": (8, 64, 32, 64, 32, 0.2), "r64": (8, 96, 32, 128, 64, 0.2)}
MLA_DECODE_LENS, MLA_KV_LENS, MLA_Q_LENS = [1, 0, 130, 300], [0, 150, 300], [0, 40, 130]


@functools.lru_cache(maxsize=None)
def mla_case(name, prefill):
    h, nope, rope, vd, r, wscale = MLA_GEOMS[name]
    kv_lens = MLA_KV_LENS if prefill else MLA_DECODE_LENS
    ckv, kpe, table, w, sk = make_mla(kv_lens, h, nope, rope, vd, r, 16, True, seed=r, wscale=wscale)
    hidden = poisoned_spare([ckv, kpe], table)
    g = torch.Generator().manual_seed(r)
    q = torch.randn(sum(MLA_Q_LENS) if prefill else len(kv_lens), h, nope + rope, generator=g).to(torch.bfloat16)
    if prefill:
        ref = build_mla("MojoPagedPrefillMLA", h, nope, rope, vd, r, True, w, sk, "cpu", is_causal=True)
        want = ref(q, ckv, kpe, cu(MLA_Q_LENS), table, cu_total_seq_lens=cu(kv_lens))
        exact = exact_mla(q, ckv, kpe, table, w, sk, h, nope, rope, vd, r, kv_lens, q_off=cu(MLA_Q_LENS).tolist())
    else:
        ref = build_mla("MojoPagedDecodeMLA", h, nope, rope, vd, r, True, w, sk, "cpu")
        want = ref(q, ckv, kpe, torch.tensor(kv_lens, dtype=torch.int32), table)
        exact = exact_mla(q, ckv, kpe, table, w, sk, h, nope, rope, vd, r, kv_lens)
    return (q, ckv, kpe, table, w, sk, hidden), want, exact


@pytest.mark.parametrize("layout", MLA_LAYOUTS, ids=MLA_LAYOUT_IDS)
@pytest.mark.parametrize("kind", ["decode", "prefill"])
@pytest.mark.parametrize("name", list(MLA_GEOMS))
def test_mla(name, kind, layout):
    h, nope, rope, vd, r, _ = MLA_GEOMS[name]
    prefill = kind == "prefill"
    (q, ckv, kpe, table, w, sk, hidden), want, exact = mla_case(name, prefill)
    caches = CL.lay_out_mla(ckv, kpe, layout[0]).to(DEV)
    tb = CL.lay_out_table(table, layout[1], hidden).to(DEV)
    qd = q.to(DEV)
    if prefill:
        op = build_mla("MojoPagedPrefillMLA", h, nope, rope, vd, r, True, w, sk, DEV, is_causal=True)
        cq, ck = cu(MLA_Q_LENS).to(DEV), cu(MLA_KV_LENS).to(DEV)
        call = lambda c, p, t: op(qd, c, p, cq, t, cu_total_seq_lens=ck)  # noqa: E731
        route = prefill_route(h, nope, rope, vd, q.shape[0])
    else:
        op = build_mla("MojoPagedDecodeMLA", h, nope, rope, vd, r, True, w, sk, DEV)
        ld = torch.tensor(MLA_DECODE_LENS, dtype=torch.int32, device=DEV)
        call = lambda c, p, t: op(qd, c, p, ld, t)  # noqa: E731
        route = "absorbed"
    forms = []

    def traced(*a):                                            # every kernel form of the call, not only the last one
        box = []
        forms.append(launches_of(lambda: box.append(call(*a))))
        return box[0]

    got, dense, _ = on_views_and_dense(traced, caches, tb)
    assert all(("mla_prefill_attn" if route == "decompress" else "mla") in f for f in forms), forms     # (c)
    out = to_cpu(got)
    assert bool(torch.isfinite(out.float()).all()), "poison was read"                                   # (d)
    check_mla(out, want, exact, route)                                                                   # (a)
    assert torch.equal(got, dense), forms                                                                # (b)


# ---- stores -----------------------------------------------------------------------------------------------------------
def check_store(hip_call, ref_call, caches_cpu, table_cpu):
    """(a), (b), (e) for a store: ``*_call(*cache views, table view)`` writes in place.  The oracle runs on a CPU clone of
    the very storage the device gets; afterwards the two storages are equal everywhere, padding and hidden pages included."""
    ref_caches, ref_table = caches_cpu.clone(), table_cpu.clone()
    ref_call(*ref_caches.views, ref_table.views[0])
    dev_caches, dev_table = caches_cpu.to(DEV), table_cpu.to(DEV)
    dense = [c.contiguous().clone() for c in dev_caches.views]
    hip_call(*dev_caches.views, dev_table.views[0])
    hip_call(*dense, dev_table.views[0].contiguous())
    torch.cuda.synchronize()
    assert any(not bit_equal(a, b) for a, b in zip(ref_caches.storages, caches_cpu.storages)), "nothing was stored"
    for got, want in zip(dev_caches.storages, ref_caches.storages):
        assert bit_equal(to_cpu(got), want)                                                            # (a), (e)
    for got, d in zip(dev_caches.views, dense):
        assert bit_equal(got, d)                                                                       # (b)
    for got, want in zip(dev_table.storages, ref_table.storages):
        assert torch.equal(to_cpu(got), want)


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("form", ["plan", "legacy"])
@pytest.mark.parametrize("which", ["fp16_page8", "bf16_page16", "decode"])
def test_store_paged_kv(which, form, layout):
    seqs, hkv, d, page, dtype = {"fp16_page8": ([(3, 9), (8, 8), (0, 24), (7, 1)], 2, 96, 8, torch.float16),
                                 "bf16_page16": ([(0, 70), (30, 33), (5, 0), (-1, 9)], 2, 128, 16, torch.bfloat16),
                                 "decode": ([(100, 1), (0, 1), (47, 1), (-1, 1), (17, 1)], 8, 128, 16, torch.bfloat16)}[which]
    ks, vs, kc, vc, table, cu_q, ctx = _store_case(seqs, hkv, d, page, dtype, seed=len(seqs))
    if which == "decode":
        ks, vs, cu_q = ks[: len(seqs)], vs[: len(seqs)], None
    hidden = poisoned_spare([kc, vc], table)
    caches, tb = CL.lay_out_kv(kc, vc, layout[0]), CL.lay_out_table(table, layout[1], hidden)
    ref, op = torch_cls("MojoStorePagedKVCache")(), hip_cls("MojoStorePagedKVCache")()
    dev = lambda t: None if t is None else t.to(DEV)  # noqa: E731
    if form == "plan":
        plan = build_paged_kv_chunk_metadata(table, cu_q, ctx, page)
        check_store(lambda a, b, t: op(dev(ks), dev(vs), a, b, chunk_metadata=plan.to(DEV)),
                    lambda a, b, t: ref(ks, vs, a, b, chunk_metadata=plan), caches, tb)
    else:
        check_store(lambda a, b, t: op(dev(ks), dev(vs), a, b, t, dev(cu_q), dev(ctx)),
                    lambda a, b, t: ref(ks, vs, a, b, t, cu_q, ctx), caches, tb)


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("form", ["plan", "legacy"])
@pytest.mark.parametrize("pattern", [0, 2, 13], ids=["prefill", "cached", "empty_row"])
def test_store_paged_kv_int8(pattern, form, layout):
    ks, vs, kc, vc, ksc, vsc, table, cu_q, ctx = c8_store_case(STORE_PATTERNS[pattern], torch.bfloat16, torch.float32, seed=pattern)
    hidden = poisoned_spare([kc, vc], table)
    caches, tb = CL.lay_out_kv(kc, vc, layout[0]), CL.lay_out_table(table, layout[1], hidden)
    ref, op = torch_cls("MojoStorePagedKVCacheC8")(), hip_cls("MojoStorePagedKVCacheC8")()
    dev = lambda t: None if t is None else t.to(DEV)  # noqa: E731
    if form == "plan":
        plan = build_paged_kv_chunk_metadata(table, cu_q, ctx, STORE_PATTERNS[pattern][3])
        check_store(lambda a, b, t: op(dev(ks), dev(vs), a, b, dev(ksc), dev(vsc), chunk_metadata=plan.to(DEV)),
                    lambda a, b, t: ref(ks, vs, a, b, ksc, vsc, chunk_metadata=plan), caches, tb)
    else:
        check_store(lambda a, b, t: op(dev(ks), dev(vs), a, b, dev(ksc), dev(vsc), t, dev(cu_q), dev(ctx)),
                    lambda a, b, t: ref(ks, vs, a, b, ksc, vsc, t, cu_q, ctx), caches, tb)


@pytest.mark.parametrize("layout", MLA_LAYOUTS, ids=MLA_LAYOUT_IDS)
@pytest.mark.parametrize("decode", [True, False], ids=["decode", "prefill"])
@pytest.mark.parametrize("geom", [(7, 16, 512, 64), (5, 128, 64, 32)], ids=["r512", "r64_page128"])
def test_store_paged_mla(geom, decode, layout):
    batch, page, r, rope = geom
    ckv, kpe, ckv_c, kpe_c, table, cu_q, ctx = mla_store_scenario(batch, page, r, rope, decode, seed=batch * 31 + page)
    hidden = poisoned_spare([ckv_c, kpe_c], table)
    caches, tb = CL.lay_out_mla(ckv_c, kpe_c, layout[0]), CL.lay_out_table(table, layout[1], hidden)
    ref, op = torch_cls("MojoStorePagedMLAKVCache")(), hip_cls("MojoStorePagedMLAKVCache")()
    dev = lambda t: None if t is None else t.to(DEV)  # noqa: E731
    check_store(lambda a, b, t: op(dev(ckv), dev(kpe), a, b, t, dev(cu_q), dev(ctx)),
                lambda a, b, t: ref(ckv, kpe, a, b, t, cu_q, ctx), caches, tb)


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_fused_qkv_rope_store(layout):
    """`qkv_rope_store` has no bit-exact CPU oracle of its own (its parity with the separate calls and the oracle's chain is
    tests/test_hip_gemm_skinny.py): here the dense call is the reference — same query bits, same cache bits inside the
    views, and not one byte of the storage changed outside them."""
    from mojo_opset_amd.backends.hip.operators.gemm import qkv_rope_store
    b, kdim, hq, hkv, d, page, pages_per_seq = 5, 1024, 8, 2, 64, 8, 6
    g = torch.Generator().manual_seed(b * 7 + d)
    n = (hq + 2 * hkv) * d
    x = torch.randn(b, kdim, generator=g).bfloat16()
    w = (torch.randn(n, kdim, generator=g) / kdim ** 0.5).bfloat16()
    bias = torch.randn(n, generator=g).bfloat16()
    cos, sin = torch.randn(b, d, generator=g), torch.randn(b, d, generator=g)
    n_blocks = b * pages_per_seq + 3
    table = torch.randperm(n_blocks, generator=g)[: b * pages_per_seq].view(b, pages_per_seq).to(torch.int32)
    ctx = torch.randint(0, pages_per_seq * page, (b,), generator=g).to(torch.int32)
    ctx[1] = -1                                               # a padded row: nothing stored
    table[2, int(ctx[2]) // page] = -1                        # a hole in the table: nothing stored
    kc = torch.randn(n_blocks, hkv, page, d, generator=g).bfloat16()
    vc = torch.randn(n_blocks, hkv, page, d, generator=g).bfloat16()
    hidden = poisoned_spare([kc, vc], table)
    caches, tb = lay_kv(kc, vc, table, hidden, layout)
    before = caches.clone()
    dense = [c.contiguous().clone() for c in caches.views]
    args = [t.to(DEV) for t in (x, w, bias, cos, sin)]
    q_got = qkv_rope_store(*args, *caches.views, tb.views[0], ctx.to(DEV), hq, hkv)
    q_dense = qkv_rope_store(*args, *dense, tb.views[0].contiguous(), ctx.to(DEV), hq, hkv)
    torch.cuda.synchronize()
    assert torch.equal(q_got, q_dense) and bool(torch.isfinite(q_got.float()).all())
    assert not bit_equal(dense[0], before.views[0])           # (something was stored)
    for got, d_ in zip(caches.views, dense):
        assert bit_equal(got, d_)
    for view, d_ in zip(before.views, dense):                 # the storage changed where the dense cache did, nowhere else
        view.copy_(d_)
    assert all(bit_equal(a, b_) for a, b_ in zip(caches.storages, before.storages))


def test_store_accepts_rows_padded_by_four_bytes():
    """The 16-bit store is the one op whose envelope is wider than 16-byte strides: its copy narrows its vectors to what
    the strides allow.  A cache whose rows are padded by two elements stores bit-exactly, padding untouched."""
    ks, vs, kc, vc, table, cu_q, ctx = _store_case([(3, 9), (8, 8), (0, 24), (7, 1)], 2, 96, 8, torch.float16, seed=4)
    n, h, page, d = kc.shape

    def narrow(t):
        s = torch.full((n, h, page, d + 2), float("nan"), dtype=t.dtype)
        s[..., :d] = t
        return s

    caches = CL.Laid([narrow(kc), narrow(vc)], lambda a, b: (a[..., :d], b[..., :d]))
    assert not CL.in_envelope(caches.views[0])
    ref, op = torch_cls("MojoStorePagedKVCache")(), hip_cls("MojoStorePagedKVCache")()
    check_store(lambda a, b, t: op(ks.to(DEV), vs.to(DEV), a, b, t, cu_q.to(DEV), ctx.to(DEV)),
                lambda a, b, t: ref(ks, vs, a, b, t, cu_q, ctx), caches, CL.lay_out_table(table, "dense", 0))


# ---- refusals ---------------------------------------------------------------------------------------------------------
def off_envelope(t):
    """``t`` over rows padded by 8 bytes: the token stride is no multiple of 16 bytes."""
    pad = 8 // t.element_size()
    s = torch.zeros(*t.shape[:-1], t.shape[-1] + pad, dtype=t.dtype, device=t.device)
    s[..., : t.shape[-1]] = t
    view = s[..., : t.shape[-1]]
    assert (view.stride(2) * t.element_size()) % 16 == 8
    return view


REFUSALS = ["decode_gqa", "decode_swa", "prefill_gqa", "prefill_swa", "decode_kv_int8", "prefill_kv_int8", "mla_decode", "mla_prefill"]


@pytest.mark.parametrize("family", REFUSALS)
def test_a_token_stride_off_the_envelope_is_refused_on_the_host(family):
    """A token stride that is not a multiple of 16 bytes raises NotImplementedError on the host — for the GQA / SWA / int8
    ops before anything is launched (the MLA ops have projected the query by then; their attention launch is what refuses)
    — and the process keeps working: the same op on the dense cache right after.  The stores are not in the list: they
    narrow their vectors to what the strides allow (`test_store_accepts_rows_padded_by_four_bytes`)."""
    from mojo_opset_amd.backends.hip import lib
    d = DEV
    swa = dict(gqa_layout="AABB", global_window_size=4, local_window_size=64)
    if family in ("decode_gqa", "decode_swa", "prefill_gqa", "prefill_swa"):
        (q, k, v, lens, table, _), _ = decode_case(8, 2, 64, 16, BASE_LENS)
        caches, td = (k.to(d), v.to(d)), table.to(d)
        if family.startswith("decode"):
            op = hip_cls("MojoPagedDecodeGQA")() if family == "decode_gqa" else hip_cls("MojoPagedDecodeSWA")(**swa)
            call = lambda a, b: op(q.to(d), a, b, lens.to(d), td)  # noqa: E731
        else:
            op = hip_cls("MojoPagedPrefillGQA")() if family == "prefill_gqa" else hip_cls("MojoPagedPrefillSWA")(**swa)
            cu_q = cu((lens > 0).int().tolist())                                   # one query token per non-empty row
            call = lambda a, b: op(q[: int(cu_q[-1])].to(d), a, b, cu_q.to(d), td, cu_total_seq_lens=cu(lens.tolist()).to(d))  # noqa: E731
    elif family.endswith("kv_int8"):
        prefill = family == "prefill_kv_int8"
        (q, k8, ks, v8, vs, table, _), _ = kv8_case("d64_bf16", prefill)
        caches, td = (k8.to(d), v8.to(d)), table.to(d)
        if prefill:
            call = lambda a, b: hip_cls(PRE8)()(q.to(d), None, a, ks.to(d), b, vs.to(d), cu(KV8_Q_LENS).to(d), td,  # noqa: E731
                                                cu_total_seq_lens=cu(SHORT_LENS).to(d))
        else:
            call = lambda a, b: hip_cls(DEC8)()(q.to(d), None, a, ks.to(d), b, vs.to(d),  # noqa: E731
                                                torch.tensor(SHORT_LENS, dtype=torch.int32, device=d), td)
    else:
        prefill = family == "mla_prefill"
        h, nope, rope, vdim, r, _ = MLA_GEOMS["r64"]
        (q, ckv, kpe, table, w, sk, _), _, _ = mla_case("r64", prefill)
        caches, td = (ckv.to(d), kpe.to(d)), table.to(d)
        if prefill:
            op = build_mla("MojoPagedPrefillMLA", h, nope, rope, vdim, r, True, w, sk, DEV, is_causal=True)
            call = lambda a, b: op(q.to(d), a, b, cu(MLA_Q_LENS).to(d), td, cu_total_seq_lens=cu(MLA_KV_LENS).to(d))  # noqa: E731
        else:
            op = build_mla("MojoPagedDecodeMLA", h, nope, rope, vdim, r, True, w, sk, DEV)
            call = lambda a, b: op(q.to(d), a, b, torch.tensor(MLA_DECODE_LENS, dtype=torch.int32, device=d), td)  # noqa: E731
    bad = [off_envelope(c) for c in caches]
    lib.launch_history(clear=True)
    with pytest.raises(NotImplementedError):
        call(*bad)
    if not family.startswith("mla"):
        assert lib.launch_history() == "", lib.launch_history()
    out = call(*caches)                                        # the process keeps working
    torch.cuda.synchronize()
    assert lib.launch_history() != "" and bool(torch.isfinite(out.float()).all())
