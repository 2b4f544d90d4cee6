"""CPU checks of tests/cache_layouts.py: every layout is a view with the dense tensor's values and the intended strides,
inside the envelope, and the torch goldens return the same bits on the views as on dense copies (so the GPU tests of
tests/test_hip_cache_layouts.py may use one oracle result for every layout)."""
import pytest
import torch

import cache_layouts as CL
import oracle.kv_int8 as G8
import oracle.swa
from conftest import bit_equal
from hip_utils import torch_cls

N, H, PAGE, D = 5, 2, 16, 64


def dense_pair(dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.int8:
        return (torch.randint(-128, 127, (N, H, PAGE, D), generator=g, dtype=torch.int8),
                torch.randint(-128, 127, (N, H, PAGE, D), generator=g, dtype=torch.int8))
    return torch.randn(N, H, PAGE, D, generator=g).to(dtype), torch.randn(N, H, PAGE, D, generator=g).to(dtype)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.int8], ids=["bf16", "fp16", "int8"])
@pytest.mark.parametrize("layout", CL.CACHE_LAYOUTS)
def test_cache_layouts_are_views_with_the_intended_strides(layout, dtype):
    k, v = dense_pair(dtype)
    laid = CL.lay_out_kv(k, v, layout)
    kv, vv = laid.views
    assert bit_equal(kv, k) and bit_equal(vv, v) and kv.shape == k.shape
    assert kv.stride() == vv.stride() and CL.in_envelope(kv) and CL.in_envelope(vv)
    pad = CL.pad_elems(dtype)
    want = {"hnd": (H * PAGE * D, PAGE * D, D, 1), "nhd": (PAGE * H * D, D, H * D, 1),
            "kv_pool": (2 * H * PAGE * D, PAGE * D, D, 1),
            "padded": (H * (PAGE + 1) * (D + pad), (PAGE + 1) * (D + pad), D + pad, 1)}[layout]
    assert kv.stride() == want
    assert all(s.is_contiguous() for s in laid.storages)
    assert (layout == "hnd") == kv.is_contiguous()
    if layout == "kv_pool":
        assert vv.data_ptr() - kv.data_ptr() == H * PAGE * D * k.element_size()
    if layout == "padded":                           # everything outside the views is poison
        for s, view in zip(laid.storages, laid.views):
            assert view.data_ptr() - s.data_ptr() == want[0] * k.element_size()
            outside = torch.ones(s.shape, dtype=torch.bool)
            outside[1:, :, :PAGE, :D] = False
            bad = s[outside]
            assert bool((bad == 127).all()) if dtype == torch.int8 else bool(torch.isnan(bad.float()).all())
    moved = laid.to("cpu").clone()                   # (what the GPU tests do with another device)
    assert moved.views[0].stride() == kv.stride() and bit_equal(moved.views[1], v)


def test_mla_fused_row_is_one_storage():
    g = torch.Generator().manual_seed(1)
    r, rope = 64, 32
    ckv, kpe = torch.randn(N, 1, PAGE, r, generator=g).bfloat16(), torch.randn(N, 1, PAGE, rope, generator=g).bfloat16()
    laid = CL.lay_out_mla(ckv, kpe, "fused_row")
    a, b = laid.views
    assert torch.equal(a, ckv) and torch.equal(b, kpe) and len(laid.storages) == 1
    assert a.stride() == b.stride() == (PAGE * (r + rope), PAGE * (r + rope), r + rope, 1)
    assert b.data_ptr() - a.data_ptr() == 2 * r and CL.in_envelope(a) and CL.in_envelope(b)


@pytest.mark.parametrize("layout", CL.TABLE_LAYOUTS)
def test_table_layouts_hide_only_valid_ids(layout):
    table = torch.tensor([[3, 1, -1], [0, 2, 4]], dtype=torch.int32)
    laid = CL.lay_out_table(table, layout, hidden_id=5)
    (t,) = laid.views
    assert torch.equal(t, table) and t.stride(1) == 1
    wide = laid.storages[0]
    if layout == "dense":
        assert t.stride(0) == 3
        return
    c = 0 if layout == "wide" else CL.TABLE_OFFSET
    assert t.stride(0) == wide.shape[1] == 3 + c + CL.TABLE_EXTRA and t.data_ptr() - wide.data_ptr() == 4 * c
    assert c % 2 == (layout == "offset")
    hidden = torch.ones(wide.shape, dtype=torch.bool)
    hidden[:, c:c + 3] = False
    assert bool((wide[hidden] == 5).all())


# ---- the goldens on views --------------------------------------------------------------------------------------------
LENS = [33, 1, 0, 70]


def paged(dtype, seed, lens=LENS, heads=H, d=D, page=PAGE):
    g = torch.Generator().manual_seed(seed)
    need = [(n + page - 1) // page for n in lens]
    total = sum(need) + 2
    if dtype == torch.int8:
        k, ks = G8.quantize_kv_cache(torch.randn(total, heads, page, d, generator=g))
        v, vs = G8.quantize_kv_cache(torch.randn(total, heads, page, d, generator=g))
    else:
        k, v = torch.randn(total, heads, page, d, generator=g).to(dtype), torch.randn(total, heads, page, d, generator=g).to(dtype)
        ks = vs = None
    table = torch.full((len(lens), max(need)), -1, dtype=torch.int32)
    ids = torch.randperm(total, generator=g, dtype=torch.int32)
    at = 0
    for b, n in enumerate(need):
        table[b, :n] = ids[at: at + n]
        at += n
    hidden = CL.poison_page([k, v], CL.spare_pages(total, table)[0])
    return k, v, ks, vs, table, hidden, g


def cu(lens):
    return torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist(), dtype=torch.int32)


@pytest.mark.parametrize("table_layout", ["wide", "offset"])
@pytest.mark.parametrize("layout", CL.CACHE_LAYOUTS[1:])
def test_attention_goldens_return_the_same_bits_on_views(layout, table_layout):
    hq = 4
    k, v, _, _, table, hidden, g = paged(torch.bfloat16, 2)
    q = torch.randn(len(LENS), hq, D, generator=g).bfloat16()
    lens = torch.tensor(LENS, dtype=torch.int32)
    kv, vv = CL.lay_out_kv(k, v, layout).views
    (tv,) = CL.lay_out_table(table, table_layout, hidden).views
    dec = torch_cls("MojoPagedDecodeGQA")()
    assert bit_equal(dec(q, kv, vv, lens, tv), dec(q, k, v, lens, table))
    swa = oracle.swa.TorchPagedDecodeSWA(global_window_size=4, local_window_size=20)
    assert bit_equal(swa.forward(q, kv, vv, lens, tv), swa.forward(q, k, v, lens, table))
    q_lens = [20, 1, 0, 30]
    qp = torch.randn(sum(q_lens), hq, D, generator=g).bfloat16()
    pre = torch_cls("MojoPagedPrefillGQA")()
    assert bit_equal(pre(qp, kv, vv, cu(q_lens), tv, cu_total_seq_lens=cu(LENS)), pre(qp, k, v, cu(q_lens), table, cu_total_seq_lens=cu(LENS)))
    pswa = oracle.swa.TorchPagedPrefillSWA(global_window_size=4, local_window_size=20)
    assert bit_equal(pswa.forward(qp, kv, vv, cu(q_lens), tv, cu_total_seq_lens=cu(LENS)),
                     pswa.forward(qp, k, v, cu(q_lens), table, cu_total_seq_lens=cu(LENS)))
    # int8 cache
    k8, v8, ks, vs, table, hidden, g = paged(torch.int8, 3)
    kv, vv = CL.lay_out_kv(k8, v8, layout).views
    (tv,) = CL.lay_out_table(table, table_layout, hidden).views
    d8, p8 = torch_cls("MojoPagedDecodeGQAWithKVDequant")(), torch_cls("MojoPagedPrefillGQAWithKVDequant")()
    assert bit_equal(d8(q, None, kv, ks, vv, vs, lens, tv), d8(q, None, k8, ks, v8, vs, lens, table))
    assert bit_equal(p8(qp, None, kv, ks, vv, vs, cu(q_lens), tv, cu_total_seq_lens=cu(LENS)),
                     p8(qp, None, k8, ks, v8, vs, cu(q_lens), table, cu_total_seq_lens=cu(LENS)))


@pytest.mark.parametrize("table_layout", ["wide", "offset"])
def test_mla_goldens_return_the_same_bits_on_a_fused_row(table_layout):
    h, nope, rope, vd, r = 4, 64, 32, 64, 32
    g = torch.Generator().manual_seed(4)
    need = [(n + PAGE - 1) // PAGE for n in LENS]
    total = sum(need) + 2
    ckv, kpe = torch.randn(total, 1, PAGE, r, generator=g).bfloat16(), torch.randn(total, 1, PAGE, rope, generator=g).bfloat16()
    table = torch.full((len(LENS), max(need)), -1, dtype=torch.int32)
    ids = torch.randperm(total, generator=g, dtype=torch.int32)
    at = 0
    for b, n in enumerate(need):
        table[b, :n] = ids[at: at + n]
        at += n
    hidden = CL.poison_page([ckv, kpe], CL.spare_pages(total, table)[0])
    cv, pv = CL.lay_out_mla(ckv, kpe, "fused_row").views
    (tv,) = CL.lay_out_table(table, table_layout, hidden).views
    w = (torch.randn(h * (nope + vd), r, generator=g) * 0.2).bfloat16()
    lens = torch.tensor(LENS, dtype=torch.int32)
    dec = torch_cls("MojoPagedDecodeMLA")(h, nope, rope, vd, r).to(torch.bfloat16)
    pre = torch_cls("MojoPagedPrefillMLA")(h, nope, rope, vd, r, is_causal=True).to(torch.bfloat16)
    with torch.no_grad():
        dec.kv_b_proj.copy_(w)
        pre.kv_b_proj.copy_(w)
    q = torch.randn(len(LENS), h, nope + rope, generator=g).bfloat16()
    assert bit_equal(dec(q, cv, pv, lens, tv), dec(q, ckv, kpe, lens, table))
    q_lens = [20, 1, 0, 30]
    qp = torch.randn(sum(q_lens), h, nope + rope, generator=g).bfloat16()
    assert bit_equal(pre(qp, cv, pv, cu(q_lens), tv, cu_total_seq_lens=cu(LENS)), pre(qp, ckv, kpe, cu(q_lens), table, cu_total_seq_lens=cu(LENS)))


@pytest.mark.parametrize("table_layout", ["wide", "offset"])
@pytest.mark.parametrize("layout", CL.CACHE_LAYOUTS[1:])
def test_store_goldens_write_through_views_and_nowhere_else(layout, table_layout):
    """The store goldens write in place: on views they change the storage exactly where the dense call changes the dense
    cache, and nothing outside the views."""
    ctx, q_lens = [30, 0, -1, 60], [3, 1, 2, 10]
    for dtype in (torch.bfloat16, torch.int8):
        k, v, _, _, table, hidden, g = paged(dtype, 5)
        if dtype == torch.int8:
            ks = torch.randn(sum(q_lens), H, D, generator=g).bfloat16()
            vs = torch.randn(sum(q_lens), H, D, generator=g).bfloat16()
            scales = (torch.rand(2, H, D, generator=g) * 0.05 + 0.01).bfloat16()
            ref = torch_cls("MojoStorePagedKVCacheC8")()
            call = lambda kc, vc, t: ref(ks, vs, kc, vc, scales[0], scales[1], t, cu(q_lens), torch.tensor(ctx, dtype=torch.int32))  # noqa: E731
        else:
            ks = torch.randn(sum(q_lens), H, D, generator=g).to(dtype)
            vs = torch.randn(sum(q_lens), H, D, generator=g).to(dtype)
            ref = torch_cls("MojoStorePagedKVCache")()
            call = lambda kc, vc, t: ref(ks, vs, kc, vc, t, cu(q_lens), torch.tensor(ctx, dtype=torch.int32))  # noqa: E731
        want = call(k.clone(), v.clone(), table)
        assert not bit_equal(want[0], k)
        laid = CL.lay_out_kv(k, v, layout)
        before = laid.clone()
        (tv,) = CL.lay_out_table(table, table_layout, hidden).views
        got = call(*laid.views, tv)
        assert bit_equal(got[0], want[0]) and bit_equal(got[1], want[1])
        assert bit_equal(laid.views[0], want[0]) and bit_equal(laid.views[1], want[1])      # written in place
        for view, w_ in zip(before.views, want):                                           # and nowhere else
            view.copy_(w_)
        assert all(bit_equal(a, b) for a, b in zip(laid.storages, before.storages))


def test_mla_store_golden_writes_through_a_fused_row():
    r, rope = 64, 32
    g = torch.Generator().manual_seed(6)
    ctx, q_lens = torch.tensor([30, 0, -1, 60], dtype=torch.int32), [3, 1, 2, 10]
    need = [(max(c, 0) + n + PAGE - 1) // PAGE for c, n in zip(ctx.tolist(), q_lens)]
    total = sum(need) + 2
    table = torch.full((4, max(need)), -1, dtype=torch.int32)
    ids = torch.randperm(total, generator=g, dtype=torch.int32)
    at = 0
    for b, n in enumerate(need):
        table[b, :n] = ids[at: at + n]
        at += n
    ckv_c, kpe_c = torch.randn(total, 1, PAGE, r, generator=g).bfloat16(), torch.randn(total, 1, PAGE, rope, generator=g).bfloat16()
    ckv, kpe = torch.randn(sum(q_lens), r, generator=g).bfloat16(), torch.randn(sum(q_lens), rope, generator=g).bfloat16()
    ref = torch_cls("MojoStorePagedMLAKVCache")()
    want = ref(ckv, kpe, ckv_c.clone(), kpe_c.clone(), table, cu(q_lens), ctx)
    laid = CL.lay_out_mla(ckv_c, kpe_c, "fused_row")
    (tv,) = CL.lay_out_table(table, "offset", CL.spare_pages(total, table)[0]).views
    ref(ckv, kpe, *laid.views, tv, cu(q_lens), ctx)
    assert torch.equal(laid.storages[0], torch.cat(list(want), dim=3)) and not torch.equal(want[0], ckv_c)
