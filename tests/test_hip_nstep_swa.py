"""GPU parity of the n-step paged decode (`MojoPagedDecodeNstepSWA`) through the C ABI.

Tolerance: atol = rtol = 2e-2, the reference's own bound for this op (test_attention.py:1775-1776) and the one
tests/test_hip_swa.py uses.  The oracle is tests/nstep_golden.py on CPU (pinned to the reference by
tests/test_nstep_golden.py).  Rows with ``0 < len < S`` and rows with holes are outside what the golden defines (NaN, and
indexing with a negative id): they are checked against the zeros the hip class promises and against the single-step hip op.
Shapes are small: a 16-token tile, two or three tiles per row, every staircase position inside a tile and on its edges."""
import pytest
import torch

import cache_layouts as CL
import nstep_golden
from conftest import load_golden
from hip_utils import DEV, assert_close_tree, hip_cls, last_launch, launches_of, run_hip_case, switch_env, to_cpu

pytestmark = pytest.mark.gpu
ATOL = RTOL = 2e-2
NAME = "MojoPagedDecodeNstepSWA"


def inputs(kv_lens, steps, hq=8, hkv=2, d=128, page=16, dtype=torch.bfloat16, seed=0):
    g = torch.Generator().manual_seed(seed)
    need = [(n + page - 1) // page for n in kv_lens]
    total = sum(need) + 3
    k = torch.randn(total, hkv, page, d, generator=g).to(dtype)
    v = torch.randn(total, hkv, page, d, generator=g).to(dtype)
    table = torch.full((len(kv_lens), max(max(need), 1)), -1, dtype=torch.int32)
    free = torch.randperm(total, generator=g, dtype=torch.int32)
    at = 0
    for b, n in enumerate(need):
        table[b, :n] = free[at: at + n]
        at += n
    q = torch.randn(len(kv_lens), steps, hq, d, generator=g).to(dtype)
    return q, k, v, torch.tensor(kv_lens, dtype=torch.int32), table


def ops(layout="AABB", glob=None, local=None):
    kw = dict(gqa_layout=layout, global_window_size=glob, local_window_size=local)
    return hip_cls(NAME)(**kw), nstep_golden.TorchPagedDecodeNstepSWA(**kw)


def on_gpu(op, args, **kw):
    out = op.forward(*[a.to(DEV) for a in args], **kw)
    torch.cuda.synchronize()
    return out


def check(kv_lens, steps, layout="AABB", glob=None, local=None, fused=True, **shape):
    """Rows of ``kv_lens`` (each 0 or >= steps) against the CPU golden; returns the output and the launch tag."""
    args = inputs(kv_lens, steps, **shape)
    hip, ref = ops(layout, glob, local)
    got = on_gpu(hip, args)
    tag = last_launch()
    if steps > 1:
        assert tag.endswith(":nstep") == fused, tag
    assert_close_tree(to_cpu(got), ref.forward(*args), ATOL, RTOL)
    return got, tag


@pytest.mark.parametrize("case", [pytest.param(c, id=str(i)) for i, c in enumerate(load_golden("paged_nstep_swa"))])
def test_captured_vectors(case):
    assert_close_tree(to_cpu(run_hip_case(case)), case["out"], ATOL, RTOL)


# (S, Hq, Hkv): 16 columns, all used; 8 q / 1 kv: one block of two steps, then two blocks with the second half filled;
# 12 columns (four lanes of sixteen idle); two columns per step; one step
GRID = [(4, 8, 2), (2, 8, 1), (3, 8, 1), (4, 6, 2), (2, 2, 2), (1, 8, 2)]


@pytest.mark.parametrize("page", [16, 128])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("steps,hq,hkv", GRID, ids=lambda v: str(v))
def test_geometry_grid(steps, hq, hkv, d, page):
    for dtype in (torch.bfloat16, torch.float16):
        for layout in ("ABAB", "AABB"):
            got, _ = check([37, 16 + steps, steps, 0, 130], steps, layout, hq=hq, hkv=hkv, d=d, page=page, dtype=dtype,
                           seed=steps * 100 + hq)
            assert not bool(got[3].any())


@pytest.mark.parametrize("steps", [2, 3, 4])
def test_staircase_across_and_on_tile_and_page_boundaries(steps):
    """The last S - 1 keys, which the earlier steps must not see, inside a tile, across a tile / page boundary, and
    starting exactly on one."""
    check([16, 17, 18, 19, 32, 33, steps, 0], steps, page=16)
    check([16, 17, 18, 19, 32, 33, steps, 0], steps, "ABAB", hq=8, hkv=1, d=64, page=16)


@pytest.mark.parametrize("glob,local", [(None, None), (4, 5), (None, 0), (2, None), (4, 255)],
                         ids=lambda v: str(v))
@pytest.mark.parametrize("steps", [2, 4])
def test_windows(steps, glob, local):
    """The local window's lower edge is a staircase too: lengths that put it across a tile boundary."""
    lens = [40, 47, 48, 49, 300, steps, 0]
    check(lens, steps, "AABB", glob, local)
    check(lens, steps, "ABAB", glob, local, hq=8, hkv=1, d=64, page=32)


def test_launch_forms():
    _, tag = check([300, 140], 4)                                       # 3 chunks of 128 tokens in one workgroup
    assert tag.startswith("decode_mfma:fused:"), tag
    _, tag = check([2100], 4, hq=4, hkv=1, glob=4, local=2060)          # 17 chunks: eight-wave workgroups + merge
    assert tag.startswith("decode_mfma:grouped+merge:"), tag
    with switch_env(MOJO_HIP_DECODE_GROUPED="0"):
        _, tag = check([2100, 5, 0, 130], 3, hq=8, hkv=1)               # single-wave workgroups + merge, two step blocks
        assert tag.startswith("decode_mfma:split+merge:"), tag
    with switch_env(MOJO_HIP_DECODE_FUSE="0"):
        _, tag = check([300, 4, 0], 4, local=200)
        assert tag.startswith("decode_mfma:split+merge:"), tag


def test_one_step_is_the_single_step_op_bit_for_bit():
    q, k, v, lens, table = inputs([700, 300, 1, 0], 1)
    for glob, local in [(None, None), (4, 255)]:
        kw = dict(gqa_layout="ABAB", global_window_size=glob, local_window_size=local)
        ref = on_gpu(hip_cls("MojoPagedDecodeSWA")(**kw), (q[:, 0].contiguous(), k, v, lens, table))
        single_tag = last_launch()
        got = on_gpu(hip_cls(NAME)(**kw), (q, k, v, lens, table))
        assert last_launch() == single_tag
        assert torch.equal(got[:, 0], ref)


@pytest.mark.parametrize("glob,local", [(None, None), (4, 37)], ids=lambda v: str(v))
def test_fused_against_composed(glob, local):
    args = inputs([300, 47, 4, 0, 131], 4)
    hip, ref = ops("AABB", glob, local)
    fused = on_gpu(hip, args)
    fused_tags = launches_of(lambda: on_gpu(hip, args))
    with switch_env(MOJO_HIP_DECODE_MFMA="0"):
        composed = on_gpu(hip, args)
        composed_tags = launches_of(lambda: on_gpu(hip, args))
    assert fused_tags.endswith(":nstep") and fused_tags.count("|") == 0, fused_tags
    assert ":nstep" not in composed_tags and composed_tags.count("decode_valu") == 4, composed_tags
    torch.testing.assert_close(fused.float(), composed.float(), atol=ATOL, rtol=RTOL)
    assert_close_tree(to_cpu(composed), ref.forward(*args), ATOL, RTOL)


@pytest.mark.parametrize("d,page", [(96, 16), (128, 48)])
def test_geometries_of_the_composed_route(d, page):
    _, tag = check([100, 50, 3, 0], 3, "ABAB", 4, 20, fused=False, d=d, page=page)
    assert ":nstep" not in tag
    check([100, 50, 3, 0], 3, "AABB", fused=False, d=d, page=page)


@pytest.mark.parametrize("mfma", [None, "0"], ids=["fused", "composed"])
def test_rows_shorter_than_their_steps(mfma):
    """``0 < len < S``: the first ``S - len`` steps see no key and store zeros; the others are the golden on those steps."""
    steps = 4
    q, k, v, lens, table = inputs([3, 1, 2, 40, 0], steps)
    for glob, local in [(None, None), (1, 1)]:
        hip, ref = ops("AABB", glob, local)
        with switch_env(MOJO_HIP_DECODE_MFMA=mfma):
            got = to_cpu(on_gpu(hip, (q, k, v, lens, table)))
        for b, n in enumerate(lens.tolist()):
            dead = max(steps - n, 0) if n > 0 else steps
            assert not bool(got[b, :dead].any()), (b, n)
            if n > 0:
                want = ref.forward(q[b:b + 1, dead:], k, v, lens[b:b + 1], table[b:b + 1])
                assert_close_tree(got[b:b + 1, dead:], want, ATOL, RTOL)


def test_validate_refuses_rows_shorter_than_their_steps(monkeypatch):
    monkeypatch.setenv("MOJO_HIP_VALIDATE", "1")
    q, k, v, lens, table = inputs([3, 40], 4)
    with pytest.raises(ValueError, match="fewer keys"):
        on_gpu(ops()[0], (q, k, v, lens, table))
    on_gpu(ops()[0], inputs([4, 40], 4))


def test_a_hole_row_is_the_single_step_op_step_by_step():
    """Negative page ids: zero K/V from the first hole on, as in `HIPPagedDecodeGQA` (no window, where the golden would
    index the cache with them)."""
    steps = 4
    q, k, v, lens, table = inputs([300, 70, 33], steps)
    table[0, 5] = -1
    table[1, 2] = -1
    got = on_gpu(ops("ABAB")[0], (q, k, v, lens, table))
    assert last_launch().endswith(":nstep")
    single = hip_cls("MojoPagedDecodeGQA")(gqa_layout="ABAB")
    for j in range(steps):
        want = on_gpu(single, (q[:, j].contiguous(), k, v, lens - (steps - 1 - j), table))
        torch.testing.assert_close(got[:, j].float(), want.float(), atol=ATOL, rtol=RTOL)


@pytest.mark.parametrize("layout", [("nhd", "dense"), ("hnd", "offset"), ("padded", "wide")], ids="-".join)
def test_strided_cache_and_table_layouts(layout):
    steps = 4
    q, k, v, lens, table = inputs([300, 47, 4, 0], steps)
    hidden = CL.poison_page([k, v], CL.spare_pages(k.shape[0], table)[0])
    caches, tb = CL.lay_out_kv(k, v, layout[0]).to(DEV), CL.lay_out_table(table, layout[1], hidden).to(DEV)
    hip, ref = ops("AABB", 4, 100)
    got = hip.forward(q.to(DEV), *caches.views, lens.to(DEV), tb.views[0])
    torch.cuda.synchronize()
    assert last_launch().endswith(":nstep")
    assert_close_tree(to_cpu(got), ref.forward(q, k, v, lens, table), ATOL, RTOL)


def test_graph_replay_with_new_lengths_leaves_padded_rows_untouched():
    steps = 4
    q, k, v, lens, table = (x.to(DEV) for x in inputs([300, 200, 130, 90], steps))
    hip, ref = ops("AABB", 4, 100)
    hip.forward(q, k, v, lens, table)                                   # warm-up (library load, attributes)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            out = hip.forward(q, k, v, lens, table, max_total_seq_len=300)
    out.fill_(7.0)
    lens.copy_(torch.tensor([290, 0, 77, 0], dtype=torch.int32, device=DEV))
    graph.replay()
    torch.cuda.synchronize()
    want = ref.forward(q.cpu(), k.cpu(), v.cpu(), lens.cpu(), table.cpu())
    got = out.cpu()
    assert bool((got[1] == 7.0).all()) and bool((got[3] == 7.0).all())
    assert_close_tree(got[[0, 2]], want[[0, 2]], ATOL, RTOL)
