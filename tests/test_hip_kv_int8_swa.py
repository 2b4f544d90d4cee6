"""GPU parity of sliding-window attention over the int8 paged KV cache (`MojoPagedDecodeSWAWithKVDequant`,
`MojoPagedPrefillSWAWithKVDequant`) through the C ABI; oracle = oracle/kv_int8_swa.py on CPU.

atol = rtol = 2e-2 on every element: the project's bound for the same kernel arithmetic in tests/test_hip_kv_int8.py
(tighter than the reference's 5e-2 on 90 % of the elements for this decode op).

Table entries outside a row's visible set are only ever set to -1 or to other valid ids: the decode kernel does not bound
page ids."""
import math

import pytest
import torch

import oracle  # noqa: F401  (registers the torch backends)
from conftest import load_golden
from hip_utils import DEV, assert_close_tree, hip_cls, last_launch, run_hip_case, switch_env, to_cpu, torch_cls
from test_hip_kv_int8 import cu, dev, make_inputs

pytestmark = pytest.mark.gpu
ATOL = RTOL = 2e-2
DEC, PRE = "MojoPagedDecodeSWAWithKVDequant", "MojoPagedPrefillSWAWithKVDequant"
WINDOWS = [("ABAB", 4, 255), ("AABB", 4, 1023)]          # the reference's windows


def check(got, want, what=""):
    diff = (got.float() - want.float()).abs()
    print(f"{what}: max |diff| {float(diff.max()) if diff.numel() else 0.0:.5f}")
    assert bool(torch.isfinite(got.float()).all()), what
    assert_close_tree(got, want, ATOL, RTOL)


def ops(name, layout, glob, local, dtype=torch.bfloat16):
    kw = dict(gqa_layout=layout, global_window_size=glob, local_window_size=local)
    ref = torch_cls(name)(**kw)
    ref.query_dtype = dtype                      # (the constructor admits bf16 only; the forward's math is dtype-generic)
    return hip_cls(name)(**kw), ref


def run_decode(op, q, k8, ks, v8, vs, lens, table, windowed=True, **kw):
    out = op(*dev(q, None, k8, ks, v8, vs, lens, table), **kw)
    torch.cuda.synchronize()
    form = last_launch()
    assert form.startswith("decode_mfma:") and ":kv8" in form and form.endswith(":swa") == windowed, form
    return out


def check_decode(layout, glob, local, lens, hq=8, hkv=2, d=128, page=16, seed=0, dtype=torch.bfloat16, **kw):
    q, k8, ks, v8, vs, table = make_inputs(hq, hkv, d, page, lens, len(lens), seed=seed, dtype=dtype)
    lens_t = torch.tensor(lens, dtype=torch.int32)
    op, ref = ops(DEC, layout, glob, local, dtype)
    got = to_cpu(run_decode(op, q, k8, ks, v8, vs, lens_t, table, **kw))
    check(got, ref(q, None, k8, ks, v8, vs, lens_t, table), f"decode {layout} g={glob} l={local} {lens}")
    return got


def run_prefill(op, q, k8, ks, v8, vs, q_lens, kv_lens, table, windowed=True, **kw):
    out = op(*dev(q, None, k8, ks, v8, vs, cu(q_lens), table), cu_total_seq_lens=cu(kv_lens).to(DEV), **kw)
    torch.cuda.synchronize()
    assert last_launch().startswith("gather:kv8:swa+" if windowed else "gather:kv8+"), last_launch()
    return out


def check_prefill(layout, glob, local, kv_lens, q_lens, hq=8, hkv=2, d=128, page=16, seed=0, dtype=torch.bfloat16, **kw):
    q, k8, ks, v8, vs, table = make_inputs(hq, hkv, d, page, kv_lens, sum(q_lens), seed=seed, dtype=dtype)
    op, ref = ops(PRE, layout, glob, local, dtype)
    got = to_cpu(run_prefill(op, q, k8, ks, v8, vs, q_lens, kv_lens, table, **kw))
    want = ref(q, None, k8, ks, v8, vs, cu(q_lens), table, cu_total_seq_lens=cu(kv_lens))
    check(got, want, f"prefill {layout} g={glob} l={local} kv={kv_lens} q={q_lens}")
    return got


# ---- recorded vectors -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [pytest.param(c, id=f"{c['op'][9:16]}-{i}") for i, c in enumerate(
    load_golden("paged_kv_int8_swa_decode") + load_golden("paged_kv_int8_swa_prefill"))
    if c["ctor"]["kwargs"]["compute_dtype"] != torch.int8])
def test_recorded_vectors(case):
    check(to_cpu(run_hip_case(case)), case["out"], case["op"])
    assert ":kv8" in last_launch() and ":swa" in last_launch(), last_launch()


# ---- decode -----------------------------------------------------------------------------------------------------------
EDGE_LENS = [1, 16, 17, 31, 32, 33, 100, 257]
EDGE_LOCALS = [0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127]


@pytest.mark.parametrize("glob", [None, 4, 16, 20])
def test_decode_window_edges(glob):
    """Window edges on, one short of and one past the 16-token sub-tile and the 32-token step: a global range of 16 keys
    (g_al = 16) puts the last global and the first local sub-tile into one step, small windows put g1 and lo into one
    sub-tile, ``local=0`` leaves the query's own key alone."""
    q, k8, ks, v8, vs, table = make_inputs(8, 2, 128, 16, EDGE_LENS, len(EDGE_LENS), seed=3)
    lens_t = torch.tensor(EDGE_LENS, dtype=torch.int32)
    for local in EDGE_LOCALS:
        op, ref = ops(DEC, "AABB", glob, local)
        got = to_cpu(run_decode(op, q, k8, ks, v8, vs, lens_t, table))
        check(got, ref(q, None, k8, ks, v8, vs, lens_t, table), f"edges g={glob} l={local}")


def test_decode_overlapping_ranges_collapse():
    check_decode("AABB", 200, 63, [150, 260])
    check_decode("ABAB", 4, 5000, [150, 260, 700])             # a local window wider than the row


ENVELOPE = [(4, 4, 64, 16), (6, 2, 80, 32), (8, 2, 96, 16), (8, 1, 128, 128), (16, 1, 128, 16), (12, 4, 64, 32)]


@pytest.mark.parametrize("layout,glob,local", WINDOWS)
@pytest.mark.parametrize("geom", ENVELOPE, ids=["D64_g1", "D80_g3_p32", "D96_g4", "D128_g8_p128", "D128_g16", "D64_g3_p32"])
def test_decode_envelope(geom, layout, glob, local):
    hq, hkv, d, page = geom
    g = torch.Generator().manual_seed(sum(geom))
    lens = torch.randint(1, 2500, (4,), generator=g).tolist()
    lens[0] = 2500
    check_decode(layout, glob, local, lens, hq=hq, hkv=hkv, d=d, page=page, seed=sum(geom))


# tile (16), step (32), minimum chunk (128) and — with 128-token chunks — chunk boundaries of the virtual length
FORM_LENS = [1, 16, 17, 32, 33, 127, 128, 129, 255, 256, 257, 300, 511, 512, 513, 1100]


@pytest.mark.parametrize("form", ["fused", "split", "chunk128"])
@pytest.mark.parametrize("glob,local", [(4, 255), (16, 111), (None, 1023)])
def test_decode_launch_forms(form, glob, local):
    env = {"fused": {}, "split": dict(MOJO_HIP_DECODE_FUSE="0"), "chunk128": dict(MOJO_HIP_DECODE_CHUNK="128")}[form]
    with switch_env(**env):
        check_decode("AABB", glob, local, FORM_LENS, seed=5)
        launched = last_launch()
    # the launch is sized on decode_swa_cap — ceil16(global) + local + 16, at most the table's capacity — in chunks of 128 tokens
    # here (32 rows of kv heads); more than 8 chunks take the split + merge form whatever the switch says
    cap = min(-(-(glob or 0) // 16) * 16 + local + 16, -(-max(FORM_LENS) // 16) * 16)
    fused = form != "split" and -(-cap // 128) <= 8
    assert ((":fused:" if fused else "split+merge") in launched), launched


def test_no_window_is_the_unwindowed_op_bit_for_bit():
    lens = [700, 3000, 1, 0]
    q, k8, ks, v8, vs, table = make_inputs(8, 2, 128, 16, lens, len(lens), seed=7)
    lens_t = torch.tensor(lens, dtype=torch.int32)
    plain = hip_cls("MojoPagedDecodeGQAWithKVDequant")(gqa_layout="ABAB")(*dev(q, None, k8, ks, v8, vs, lens_t, table))
    got = run_decode(ops(DEC, "ABAB", None, None)[0], q, k8, ks, v8, vs, lens_t, table, windowed=False)
    assert torch.equal(got, plain)
    kv_lens, q_lens = [900, 400], [300, 400]
    q, k8, ks, v8, vs, table = make_inputs(8, 2, 128, 16, kv_lens, sum(q_lens), seed=8)
    plain = hip_cls("MojoPagedPrefillGQAWithKVDequant")()(*dev(q, None, k8, ks, v8, vs, cu(q_lens), table),
                                                          cu_total_seq_lens=cu(kv_lens).to(DEV))
    got = run_prefill(ops(PRE, "AABB", None, None)[0], q, k8, ks, v8, vs, q_lens, kv_lens, table, windowed=False)
    assert torch.equal(got, plain)


def spoil_outside(k8, v8, table, rows):
    """+-127 into every page no row of ``rows`` [(b, first locally visible key, global end, length)] can see, and -1 for
    their table entries."""
    k8, v8, table = k8.clone(), v8.clone(), table.clone()
    page = k8.shape[2]
    for b, lo, gend, n in rows:
        for p in range((n + page - 1) // page):
            if p * page >= gend and (p + 1) * page <= lo:
                k8[int(table[b, p])] = 127
                v8[int(table[b, p])] = -127
                table[b, p] = -1
    return k8, v8, table


@pytest.mark.parametrize("form", ["fused", "split"])
def test_decode_never_reads_pages_outside_the_window(form):
    local, glob = 255, 20
    lens = [3000, 1200, 600, 200]
    q, k8, ks, v8, vs, table = make_inputs(8, 2, 128, 16, lens, len(lens), seed=9)
    lens_t = torch.tensor(lens, dtype=torch.int32)
    op = ops(DEC, "AABB", glob, local)[0]
    k2, v2, t2 = spoil_outside(k8, v8, table, [(b, max(n - 1 - local, 0), glob, n) for b, n in enumerate(lens)])
    assert int((t2 < 0).sum()) > int((table < 0).sum())
    with switch_env(MOJO_HIP_DECODE_FUSE="0" if form == "split" else None):
        clean = run_decode(op, q, k8, ks, v8, vs, lens_t, table)
        assert ("split+merge" if form == "split" else ":fused:") in last_launch(), last_launch()
        assert torch.equal(run_decode(op, q, k2, ks, v2, vs, lens_t, t2), clean)


def test_prefill_never_reads_pages_outside_the_union():
    local, glob = 255, 20
    kv_lens, q_lens = [3000, 900, 700], [200, 100, 700]
    q, k8, ks, v8, vs, table = make_inputs(8, 2, 128, 16, kv_lens, sum(q_lens), seed=10)
    op = ops(PRE, "AABB", glob, local)[0]
    clean = run_prefill(op, q, k8, ks, v8, vs, q_lens, kv_lens, table)
    k2, v2, t2 = spoil_outside(k8, v8, table, [(b, max(n - ql - local, 0), glob, n) for b, (n, ql) in enumerate(zip(kv_lens, q_lens))])
    assert int((t2 < 0).sum()) > int((table < 0).sum())
    assert torch.equal(run_prefill(op, q, k2, ks, v2, vs, q_lens, kv_lens, t2), clean)
    assert torch.equal(run_prefill(op, q, k2, ks, v2, vs, q_lens, kv_lens, t2, max_q_len=700, max_total_seq_len=3000), clean)


def test_zero_length_rows_and_fp16():
    got = check_decode("ABAB", 4, 255, [0, 700, 0, 33], dtype=torch.float16)
    assert got.dtype == torch.float16 and not bool(got[0].any()) and not bool(got[2].any())
    check_prefill("AABB", 4, 255, [0, 600, 50], [0, 100, 50], dtype=torch.float16)


def test_graph_replay_with_new_lengths_leaves_padded_rows_untouched():
    lens = [2000, 1500, 800, 400]
    q, k8, ks, v8, vs, table = make_inputs(8, 2, 128, 16, lens, len(lens), seed=11)
    args = dev(q, None, k8, ks, v8, vs, torch.tensor(lens, dtype=torch.int32), table)
    op, ref = ops(DEC, "AABB", 4, 1023)
    op(*args)                                                            # warm-up (library load, attributes)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            out = op(*args, max_total_seq_len=2000)
    out.fill_(7.0)
    new = torch.tensor([1900, 0, 700, 0], dtype=torch.int32)
    args[6].copy_(new.to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    got = out.cpu()
    assert bool((got[1] == 7.0).all()) and bool((got[3] == 7.0).all())
    check(got[[0, 2]], ref(q, None, k8, ks, v8, vs, new, table)[[0, 2]], "replay")


# ---- prefill ----------------------------------------------------------------------------------------------------------
PREFILL_CFGS = [((1300, 700), (1300, 300), 32, 8, 128, 16), ((2100,), (400,), 16, 4, 128, 32),
                ((900, 1500), (900, 64), 8, 8, 64, 128), ((1200,), (1200,), 16, 2, 96, 16), ((700, 90), (130, 90), 8, 4, 128, 16)]


@pytest.mark.parametrize("layout,glob,local", WINDOWS)
@pytest.mark.parametrize("cfg", PREFILL_CFGS, ids=["1300+700_g4", "2100-chunk400_g4_p32", "900+1500_g1_p128", "1200_d96_g8", "700+90_g2"])
def test_prefill_config_space(cfg, layout, glob, local):
    kv_lens, q_lens, hq, hkv, d, page = cfg
    check_prefill(layout, glob, local, list(kv_lens), list(q_lens), hq=hq, hkv=hkv, d=d, page=page, seed=sum(kv_lens))
    check_prefill(layout, glob, local, list(kv_lens), list(q_lens), hq=hq, hkv=hkv, d=d, page=page, seed=sum(kv_lens),
                  max_q_len=max(q_lens), max_total_seq_len=max(kv_lens))


@pytest.mark.parametrize("local", [0, 15, 16, 17, 63, 64, 65])
def test_prefill_window_edges(local):
    """Local starts and global ends on, one short of and one past page and key-tile boundaries; global only; ranges that meet."""
    check_prefill("AABB", local + 1, local, [400, 128 + local], [200, 100], page=16, hq=4, hkv=2, seed=local)
    check_prefill("AABB", None, local, [300], [300], page=32, hq=2, hkv=2, d=64, seed=local)
    check_prefill("ABAB", 16 + local, None, [500, 33], [100, 33], page=16, hq=4, hkv=2, seed=local)
    check_prefill("AABB", 100, 150 + local, [300, 260], [300, 100], seed=local)


@pytest.mark.parametrize("ksplit", ["1", "4"])
def test_prefill_key_split(ksplit):
    with switch_env(MOJO_HIP_PREFILL_KSPLIT=ksplit):
        check_prefill("AABB", 4, 1023, [6000], [128], hq=8, hkv=2, seed=12)


def test_prefill_on_an_uninitialised_workspace():
    """The entry point on a caller-supplied workspace filled with 0xFF (NaN in both 16-bit formats), the call built as
    `_paged_prefill` builds it: no byte of scratch that the gather did not write may reach the output."""
    from mojo_opset_amd.backends.hip import lib as L

    kv_lens, q_lens, glob, local = [3000, 40, 700], [200, 40, 0], 20, 255
    hq, hkv, d, page = 8, 2, 128, 16
    q, k8, ks, v8, vs, table = make_inputs(hq, hkv, d, page, kv_lens, sum(q_lens), seed=13)
    # row 1: its first page is absent, so pool pages are addressed that nothing was gathered into
    holed = table.clone()
    holed[1, 0] = -1
    lib = L.load()
    first = None
    for tab, hints in ((table, (200, 3000)), (table, (0, 0)), (holed, (0, 0))):
        dq, dk, dks, dv, dvs, dt, cq, ckv = dev(q, k8, ks, v8, vs, tab, cu(q_lens), cu(kv_lens))
        ws_bytes = lib.mojo_hip_paged_prefill_swa_kv8_workspace_bytes(q.shape[0], len(kv_lens), hq, hkv, d, page, dt.shape[1],
                                                                      *hints, local, glob)
        ws = torch.full((ws_bytes,), 0xFF, dtype=torch.uint8, device=DEV)
        out = torch.full_like(dq, float("nan"))
        L.check(lib.mojo_hip_paged_prefill_swa_kv8(
            L.ptr(dq), L.ptr(dk), L.ptr(dks), L.ptr(dv), L.ptr(dvs), L.ptr(cq), L.ptr(ckv), L.ptr(dt), L.ptr(out),
            q.shape[0], len(kv_lens), hq, hkv, d, k8.shape[0], page, dt.shape[1], dt.stride(0), dk.stride(0), dk.stride(1),
            dk.stride(2), *hints, 1.0 / math.sqrt(d), 0, L.dtype_code(dq.dtype), L.dtype_code(dks.dtype), L.ptr(ws), ws_bytes,
            local, glob, L.stream_of(dq)), "paged_prefill_swa_kv8")
        torch.cuda.synchronize()
        got = to_cpu(out)
        assert bool(torch.isfinite(got.float()).all())
        if tab is table:
            want = ops(PRE, "AABB", glob, local)[1](q, None, k8, ks, v8, vs, cu(q_lens), table, cu_total_seq_lens=cu(kv_lens))
            check(got, want, f"0xFF workspace hints={hints}")
        else:                                                    # rows 0 and 2 are untouched by row 1's absent page
            assert torch.equal(got[:200], first[:200])
        first = got if tab is table else first
