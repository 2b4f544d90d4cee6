"""GPU parity of the sliding-window pair (`MojoPagedDecodeSWA`, `MojoPagedPrefillSWA`) through the C ABI.

Tolerance: atol = rtol = 2e-2, the reference's own bound for these ops (test_attention.py:1434-1435, :1695-1696).
The oracle is oracle/swa.py on CPU (pinned to the reference by tests/test_swa_golden.py)."""
import pytest
import torch

import oracle.swa
from conftest import build_op, load_golden
from hip_utils import DEV, assert_close_tree, hip_cls, last_launch, run_hip_case, switch_env, to_cpu

pytestmark = pytest.mark.gpu
ATOL = RTOL = 2e-2
WINDOWS = [("ABAB", 4, 255), ("AABB", 4, 1023)]


def paged(batch, hkv, d, kv_lens, page, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    need = [(n + page - 1) // page for n in kv_lens]
    total = sum(need) + 3
    k = torch.randn(total, hkv, page, d, generator=g).to(dtype)
    v = torch.randn(total, hkv, page, d, generator=g).to(dtype)
    table = torch.full((batch, max(max(need), 1)), -1, dtype=torch.int32)
    free = torch.randperm(total, generator=g, dtype=torch.int32)
    at = 0
    for b, n in enumerate(need):
        table[b, :n] = free[at: at + n]
        at += n
    return k, v, table, g


def decode_inputs(kv_lens, hq=8, hkv=2, d=128, page=16, dtype=torch.bfloat16, seed=0):
    k, v, table, g = paged(len(kv_lens), hkv, d, kv_lens, page, dtype, seed)
    q = torch.randn(len(kv_lens), hq, d, generator=g).to(dtype)
    return q, k, v, torch.tensor(kv_lens, dtype=torch.int32), table


def prefill_inputs(kv_lens, q_lens, hq=8, hkv=2, d=128, page=16, dtype=torch.bfloat16, seed=0):
    k, v, table, g = paged(len(kv_lens), hkv, d, kv_lens, page, dtype, seed)
    q = torch.randn(sum(q_lens), hq, d, generator=g).to(dtype)
    cu_q = torch.tensor([0] + torch.tensor(q_lens).cumsum(0).tolist(), dtype=torch.int32)
    cu_kv = torch.tensor([0] + torch.tensor(kv_lens).cumsum(0).tolist(), dtype=torch.int32)
    return q, k, v, cu_q, table, cu_kv


def ops(kind, layout, glob, local):
    name = "MojoPagedDecodeSWA" if kind == "decode" else "MojoPagedPrefillSWA"
    kw = dict(gqa_layout=layout, global_window_size=glob, local_window_size=local)
    return hip_cls(name)(**kw), getattr(oracle.swa, "Torch" + name[4:])(**kw)


def on_gpu(op, args, **kw):
    out = op.forward(*[a.to(DEV) if isinstance(a, torch.Tensor) else a for a in args],
                     **{k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in kw.items()})
    torch.cuda.synchronize()
    return out


def check_decode(layout, glob, local, kv_lens, **shape):
    args = decode_inputs(kv_lens, **shape)
    hip, ref = ops("decode", layout, glob, local)
    got = on_gpu(hip, args)
    assert last_launch().endswith(":swa"), last_launch()
    assert_close_tree(to_cpu(got), ref.forward(*args), ATOL, RTOL)
    return got


def check_prefill(layout, glob, local, kv_lens, q_lens, **shape):
    q, k, v, cu_q, table, cu_kv = prefill_inputs(kv_lens, q_lens, **shape)
    hip, ref = ops("prefill", layout, glob, local)
    got = on_gpu(hip, (q, k, v, cu_q, table), cu_total_seq_lens=cu_kv)
    assert last_launch().endswith(":swa"), last_launch()
    assert_close_tree(to_cpu(got), ref.forward(q, k, v, cu_q, table, cu_total_seq_lens=cu_kv), ATOL, RTOL)
    return got


@pytest.mark.parametrize("case", [pytest.param(c, id=f"{c['op'][4:]}-{i}") for i, c in
                                  enumerate(load_golden("paged_swa") + load_golden("paged_swa_prefill"))])
def test_captured_vectors(case):
    assert_close_tree(to_cpu(run_hip_case(case)), case["out"], ATOL, RTOL)


# the reference's config spaces (decode test_attention.py:1634-1642, prefill :1356-1364) inside the envelope
DECODE_CFGS = [(8, 32, 8, 128, 4096, 16), (8, 16, 4, 128, 2048, 32), (4, 32, 32, 128, 3000, 128), (4, 24, 8, 128, 2500, 1024),
               (6, 16, 2, 64, 2048, 16), (5, 8, 4, 96, 1500, 16)]
PREFILL_CFGS = [((1300, 700), (1300, 300), 32, 8, 128, 16), ((2100,), (400,), 16, 4, 128, 32),
                ((900, 1500), (900, 64), 8, 8, 64, 128), ((1200,), (1200,), 16, 2, 96, 1024),
                pytest.param(((1000,), (1000,), 24, 8, 128, 16), marks=pytest.mark.skip(
                    reason="24 q / 8 kv heads: the prefill kernel instantiates groups of 1, 2, 4 and 8 only (out of scope)"))]


@pytest.mark.parametrize("layout,glob,local", WINDOWS)
@pytest.mark.parametrize("cfg", DECODE_CFGS, ids=lambda c: "x".join(map(str, c)))
def test_decode_config_space(cfg, layout, glob, local):
    batch, hq, hkv, d, max_len, page = cfg
    g = torch.Generator().manual_seed(batch * hq + page)
    lens = torch.randint(1, max_len, (batch,), generator=g).tolist()
    lens[0] = max_len
    check_decode(layout, glob, local, lens, hq=hq, hkv=hkv, d=d, page=page)


@pytest.mark.parametrize("layout,glob,local", WINDOWS)
@pytest.mark.parametrize("cfg", PREFILL_CFGS, ids=["1300+700", "2100-chunk400", "900+1500-p128", "1200-d96-p1024", "24x8"])
def test_prefill_config_space(cfg, layout, glob, local):
    kv_lens, q_lens, hq, hkv, d, page = cfg
    check_prefill(layout, glob, local, list(kv_lens), list(q_lens), hq=hq, hkv=hkv, d=d, page=page)


@pytest.mark.parametrize("local", [1, 15, 16, 17, 63, 64, 65, 127])
def test_window_edges(local):
    """Local windows and global windows whose edges fall on, one short of and one past tile / page boundaries."""
    lens = [300, 301, 317, 64 + local, local + 1, local + 2]
    check_decode("AABB", None, local, lens, page=16)
    check_decode("ABAB", local, local, lens, page=32, hq=4, hkv=4, d=64)
    check_prefill("AABB", local, local, [400, 128 + local], [200, 100], page=16, hq=4, hkv=2)
    check_prefill("AABB", None, local, [300], [300], page=32, hq=2, hkv=2, d=64)


def test_overlapping_ranges_collapse():
    check_decode("AABB", 100, 150, [200, 240, 260, 90])
    check_prefill("AABB", 100, 150, [300, 260], [300, 100])


@pytest.mark.parametrize("env", [dict(MOJO_HIP_DECODE_MFMA="1"), dict(MOJO_HIP_DECODE_MFMA="0"),
                                 dict(MOJO_HIP_DECODE_FUSE="0"), dict(MOJO_HIP_DECODE_CHUNK="128"),
                                 dict(MOJO_HIP_DECODE_CHUNK="128", MOJO_HIP_DECODE_MFMA="0")],
                         ids=lambda e: ",".join(f"{k[9:]}={v}" for k, v in e.items()))
@pytest.mark.parametrize("d,hq,hkv", [(128, 8, 2), (64, 8, 1), (96, 4, 2)])
def test_every_decode_form(env, d, hq, hkv):
    if d == 96 and env.get("MOJO_HIP_DECODE_MFMA") == "1":
        env = dict(env, MOJO_HIP_DECODE_MFMA="0")
    with switch_env(**env):
        check_decode("AABB", 4, 1023, [5000, 1200, 3000, 20], d=d, hq=hq, hkv=hkv)
        form = last_launch()
    want = "valu" if env.get("MOJO_HIP_DECODE_MFMA") == "0" or d == 96 else "mfma"
    assert form.startswith("decode_" + want), form
    if env.get("MOJO_HIP_DECODE_FUSE") == "0" or "MOJO_HIP_DECODE_CHUNK" in env:
        assert "merge" in form, form


@pytest.mark.parametrize("env", [dict(MOJO_HIP_PREFILL_KSPLIT="1"), dict(MOJO_HIP_PREFILL_KSPLIT="4"),
                                 dict(MOJO_HIP_PREFILL_FAST_STAGE="0")], ids=lambda e: ",".join(e.values()))
def test_prefill_forms(env):
    with switch_env(**env):
        check_prefill("AABB", 4, 1023, [6000], [128], hq=8, hkv=2)
        form = last_launch()
    if env.get("MOJO_HIP_PREFILL_KSPLIT") == "4":
        assert ":ksplit4" in form
    if "MOJO_HIP_PREFILL_FAST_STAGE" in env:
        assert ":general_stage:" in form


def test_no_window_is_the_gqa_op_bit_for_bit_and_a_wide_one_is_close():
    q, k, v, lens, table = decode_inputs([700, 3000, 1, 0])
    gqa = hip_cls("MojoPagedDecodeGQA")(gqa_layout="ABAB")
    ref = on_gpu(gqa, (q, k, v, lens, table))
    assert torch.equal(on_gpu(ops("decode", "ABAB", None, None)[0], (q, k, v, lens, table)), ref)
    wide = on_gpu(ops("decode", "ABAB", None, 5000)[0], (q, k, v, lens, table))
    torch.testing.assert_close(wide.float(), ref.float(), atol=2e-3, rtol=2e-3)
    q, k, v, cu_q, table, cu_kv = prefill_inputs([900, 400], [300, 400])
    gqa = hip_cls("MojoPagedPrefillGQA")()
    ref = on_gpu(gqa, (q, k, v, cu_q, table), cu_total_seq_lens=cu_kv)
    assert torch.equal(on_gpu(ops("prefill", "AABB", None, None)[0], (q, k, v, cu_q, table), cu_total_seq_lens=cu_kv), ref)
    wide = on_gpu(ops("prefill", "AABB", None, 5000)[0], (q, k, v, cu_q, table), cu_total_seq_lens=cu_kv)
    torch.testing.assert_close(wide.float(), ref.float(), atol=2e-3, rtol=2e-3)


def _spoil_outside(k, v, table, rows):
    """NaN into every page no row of `rows` [(b, first visible key, global end, length)] can see, and -1 for their
    table entries."""
    k, v, table = k.clone(), v.clone(), table.clone()
    page = k.shape[2]
    for b, lo, gend, n in rows:
        for p in range((n + page - 1) // page):
            if p * page >= gend and (p + 1) * page <= lo:
                k[int(table[b, p])] = float("nan")
                v[int(table[b, p])] = float("nan")
                table[b, p] = -1
    return k, v, table


@pytest.mark.parametrize("mfma", ["0", "1"])
def test_pages_outside_the_window_are_never_read(mfma):
    local, glob = 255, 4
    lens = [3000, 1200, 600, 200]
    q, k, v, t_lens, table = decode_inputs(lens, d=128)
    op = ops("decode", "AABB", glob, local)[0]
    with switch_env(MOJO_HIP_DECODE_MFMA=mfma):
        clean = on_gpu(op, (q, k, v, t_lens, table))
        k2, v2, t2 = _spoil_outside(k, v, table, [(b, max(n - 1 - local, 0), glob, n) for b, n in enumerate(lens)])
        assert int((t2 < 0).sum()) > int((table < 0).sum())
        assert torch.equal(on_gpu(op, (q, k2, v2, t_lens, t2)), clean)
    kv_lens, q_lens = [3000, 900], [200, 100]
    q, k, v, cu_q, table, cu_kv = prefill_inputs(kv_lens, q_lens)
    op = ops("prefill", "AABB", glob, local)[0]
    clean = on_gpu(op, (q, k, v, cu_q, table), cu_total_seq_lens=cu_kv)
    k2, v2, t2 = _spoil_outside(k, v, table, [(b, max(n - ql - local, 0), glob, n) for b, (n, ql) in enumerate(zip(kv_lens, q_lens))])
    assert torch.equal(on_gpu(op, (q, k2, v2, cu_q, t2), cu_total_seq_lens=cu_kv), clean)


def test_graph_replay_with_new_lengths_leaves_padded_rows_untouched():
    q, k, v, lens, table = decode_inputs([2000, 1500, 800, 400])
    q, k, v, lens, table = (x.to(DEV) for x in (q, k, v, lens, table))
    op = ops("decode", "AABB", 4, 1023)[0]
    op.forward(q, k, v, lens, table)                                    # warm-up (library load, attributes)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            out = op.forward(q, k, v, lens, table, max_total_seq_len=2000)
    out.fill_(7.0)
    lens.copy_(torch.tensor([1900, 0, 700, 0], dtype=torch.int32, device=DEV))
    graph.replay()
    torch.cuda.synchronize()
    ref = ops("decode", "AABB", 4, 1023)[1].forward(q.cpu(), k.cpu(), v.cpu(), lens.cpu(), table.cpu())
    got = out.cpu()
    assert bool((got[1] == 7.0).all()) and bool((got[3] == 7.0).all())
    assert_close_tree(got[[0, 2]], ref[[0, 2]], ATOL, RTOL)


def test_zero_length_rows_and_fp16():
    got = check_decode("ABAB", 4, 255, [0, 700, 0, 33], dtype=torch.float16)
    assert not bool(got[0].any()) and not bool(got[2].any())
    got = check_prefill("AABB", 4, 255, [0, 600, 50], [10, 100, 50], dtype=torch.float16)
    assert not bool(got[:10].any())
