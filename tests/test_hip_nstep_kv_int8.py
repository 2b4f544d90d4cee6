"""GPU parity of the n-step paged decode over the int8 cache (`MojoPagedDecodeNstepSWAWithKVDequant`) through the C ABI.

Tolerance: atol = rtol = 2e-2 on every element, the project's bound for this kernel's arithmetic (tests/test_hip_kv_int8.py,
tests/test_hip_kv_int8_swa.py): the n-step kernel changes the column assignment, not the arithmetic.  The oracle is
tests/nstep_kv_int8_golden.py on the CPU (pinned to the prefill golden by tests/test_nstep_kv_int8_golden.py).  Rows with
``0 < len < S`` and rows with holes are outside what the golden defines: they are checked against the zeros the hip class
promises and against the single-step hip op.  Shapes are small: a step of the kernel is 32 tokens (two 16-token sub-tiles),
a handful of sequences of at most a few hundred tokens, every staircase position inside a sub-tile and on its edges."""
import pytest
import torch

import cache_layouts as CL
import nstep_kv_int8_golden as NG
from hip_utils import DEV, assert_close_tree, hip_cls, last_launch, launches_of, switch_env, to_cpu
from test_hip_kv_int8 import make_inputs

pytestmark = pytest.mark.gpu
ATOL = RTOL = 2e-2
NAME = "MojoPagedDecodeNstepSWAWithKVDequant"
SINGLE = "MojoPagedDecodeSWAWithKVDequant"


def inputs(kv_lens, steps, hq=8, hkv=2, d=128, page=16, dtype=torch.bfloat16, seed=0):
    """(query [B,S,Hq,D], None, k8, key_scale, v8, value_scale, lens, table): the forward's arguments."""
    q, k8, ks, v8, vs, table = make_inputs(hq, hkv, d, page, kv_lens, len(kv_lens) * steps, seed=seed, dtype=dtype, spare=3)
    return q.reshape(len(kv_lens), steps, hq, d), None, k8, ks, v8, vs, torch.tensor(kv_lens, dtype=torch.int32), table


def ops(layout="AABB", glob=None, local=None, dtype=torch.bfloat16):
    kw = dict(gqa_layout=layout, global_window_size=glob, local_window_size=local)
    ref = NG.TorchPagedDecodeNstepSWAWithKVDequant(**kw)
    ref.query_dtype = dtype                # (the constructor admits bf16 only; the forward's math is dtype-generic)
    return hip_cls(NAME)(**kw), ref


def on_gpu(op, args, **kw):
    out = op.forward(*[a if a is None else a.to(DEV) for a in args], **kw)
    torch.cuda.synchronize()
    return out


def compare(got, want, what=""):
    got = to_cpu(got)
    assert bool(torch.isfinite(got.float()).all()), what
    diff = (got.float() - want.float()).abs()
    print(f"{what}: max |diff| {float(diff.max()) if diff.numel() else 0.0:.5f}")
    assert_close_tree(got, want, ATOL, RTOL)


def check(kv_lens, steps, layout="AABB", glob=None, local=None, fused=True, hint=None, **shape):
    """Rows of ``kv_lens`` (each 0 or >= steps) against the CPU golden; returns the output and the launch tag."""
    args = inputs(kv_lens, steps, **shape)
    hip, ref = ops(layout, glob, local, args[0].dtype)
    got = on_gpu(hip, args, **({} if hint is None else {"max_total_seq_len": hint}))
    tag = last_launch()
    assert ":kv8" in tag, tag
    assert tag.endswith(":nstep") == (fused and steps > 1), tag
    compare(got, ref.forward(*args), f"S={steps} {layout} g={glob} l={local} {shape} {tag}")
    return got, tag


# (S, Hq, Hkv): 16 columns, all used; 8 q / 1 kv: one block of two steps, then two blocks with the second half filled;
# 12 columns (four lanes of sixteen idle); two columns per step; one step
GRID = [(4, 8, 2), (2, 8, 1), (3, 8, 1), (4, 6, 2), (2, 2, 2), (1, 8, 2)]


@pytest.mark.parametrize("page", [16, 48, 128])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("steps,hq,hkv", GRID, ids=lambda v: str(v))
def test_geometry_grid(steps, hq, hkv, d, page):
    for dtype in (torch.bfloat16, torch.float16):
        for layout in ("ABAB", "AABB"):
            got, _ = check([37, 16 + steps, steps, 0, 130], steps, layout, hq=hq, hkv=hkv, d=d, page=page, dtype=dtype,
                           seed=steps * 100 + hq)
            assert not bool(got[3].any())


@pytest.mark.parametrize("d", [80, 96])
def test_the_other_head_dims_of_the_int8_kernel(d):
    check([37, 20, 4, 0, 130], 4, "ABAB", 4, 20, d=d)
    check([37, 19, 3, 0, 130], 3, "AABB", hq=8, hkv=1, d=d, page=48)


@pytest.mark.parametrize("steps", [2, 3, 4])
def test_staircase_placement(steps):
    """The last S - 1 keys, which the earlier steps must not see, inside a sub-tile, across a sub-tile edge, across the edge
    of a 32-token step of the kernel (three in flight), and exactly on each."""
    lens = [16, 17, 18, 19, 31, 32, 33, 34, 64, 65, 96, 97, 98, steps, 0]
    check(lens, steps)
    check(lens, steps, "ABAB", hq=8, hkv=1, d=64)


@pytest.mark.parametrize("glob,local", [(None, None), (4, 5), (None, 0), (2, None), (4, 255), (16, 20)],
                         ids=lambda v: str(v))
@pytest.mark.parametrize("steps", [2, 4])
def test_windows(steps, glob, local):
    """The local window's lower edge is a staircase too: lengths that put it across a sub-tile edge.  (16, 20) puts the last
    global and the first local sub-tile into one step of the kernel."""
    lens = [40, 47, 48, 49, 300, steps, 0]
    check(lens, steps, "AABB", glob, local)
    check(lens, steps, "ABAB", glob, local, hq=8, hkv=1, d=64, page=32)


def planned_chunks(lib, batch, hq, hkv, d, page, pages, hint, steps):
    """Chunks per row of the launch the library plans, read off the workspace it asks for (one (d + 2)-float slot per
    chunk and column)."""
    group = hq // hkv
    sb = 16 // group
    blocks = -(-steps // sb)
    slots = (lib.mojo_hip_paged_decode_nstep_kv8_workspace_bytes(batch, hq, hkv, d, page, pages, hint, -1, 0, steps) - 256) // ((d + 2) * 4)
    return slots // (batch * hkv * blocks * sb * group)


def test_launch_forms():
    from mojo_opset_amd.backends.hip import lib as L

    _, tag = check([300, 140], 4)                                       # 3 chunks of 128 tokens in one workgroup
    assert tag.startswith("decode_mfma:fused:"), tag
    _, tag = check([300, 5, 0, 130], 3, hq=8, hkv=1)                    # two blocks of steps, fused
    assert tag.startswith("decode_mfma:fused:"), tag
    with switch_env(MOJO_HIP_DECODE_FUSE="0"):
        _, tag = check([300, 4, 0], 4, local=200)
        assert tag.startswith("decode_mfma:split+merge:"), tag
        _, tag = check([300, 5, 0, 130], 3, hq=8, hkv=1)                # two blocks of steps, split + merge
        assert tag.startswith("decode_mfma:split+merge:"), tag
    # the smallest length that plans more than 8 chunks (chunks are whole 16-token tiles, 128 tokens at the least)
    lib = L.load()
    long = next(n for n in range(129, 4097, 128) if planned_chunks(lib, 2, 4, 1, 128, 16, -(-n // 16), n, 4) > 8)
    assert planned_chunks(lib, 2, 4, 1, 128, 16, -(-(long - 128) // 16), long - 128, 4) <= 8 and long < 1200
    _, tag = check([long, 140], 4, hq=4, hkv=1, hint=long)
    assert tag.startswith("decode_mfma:split+merge:"), tag
    _, tag = check([long, 140], 4, hq=4, hkv=1, glob=4, local=long - 10)      # (visible span past the table's capacity)
    assert tag.startswith("decode_mfma:split+merge:"), tag


def test_one_step_is_the_single_step_op_bit_for_bit():
    args = inputs([700, 300, 1, 0], 1)
    single_args = (args[0][:, 0].contiguous(), *args[1:])
    for glob, local in [(None, None), (4, 255)]:
        kw = dict(gqa_layout="ABAB", global_window_size=glob, local_window_size=local)
        ref = on_gpu(hip_cls(SINGLE)(**kw), single_args)
        single_tag = last_launch()
        got = on_gpu(hip_cls(NAME)(**kw), args)
        assert last_launch() == single_tag and ":kv8" in single_tag
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
    assert fused_tags.endswith(":nstep") and ":kv8" in fused_tags and fused_tags.count("|") == 0, fused_tags
    assert ":nstep" not in composed_tags and composed_tags.count(":kv8") == 4 and composed_tags.count("|") == 3, composed_tags
    torch.testing.assert_close(fused.float(), composed.float(), atol=ATOL, rtol=RTOL)
    compare(composed, ref.forward(*args), "composed")


@pytest.mark.parametrize("mfma", [None, "0"], ids=["fused", "composed"])
def test_rows_shorter_than_their_steps(mfma):
    """``0 < len < S``: the first ``S - len`` steps see no key and store zeros; the others are the golden on those steps."""
    steps = 4
    q, _, k8, ks, v8, vs, lens, table = inputs([3, 1, 2, 40, 0], steps)
    for glob, local in [(None, None), (1, 1)]:
        hip, ref = ops("AABB", glob, local)
        with switch_env(MOJO_HIP_DECODE_MFMA=mfma):
            got = to_cpu(on_gpu(hip, (q, None, k8, ks, v8, vs, lens, table)))
            assert last_launch().endswith(":nstep") == (mfma is None)
        for b, n in enumerate(lens.tolist()):
            dead = max(steps - n, 0) if n > 0 else steps
            assert not bool(got[b, :dead].any()), (b, n)
            if n > 0:
                want = ref.forward(q[b:b + 1, dead:], None, k8, ks, v8, vs, lens[b:b + 1], table[b:b + 1])
                compare(got[b:b + 1, dead:], want, f"row {b}")


def test_validate_refuses_rows_shorter_than_their_steps(monkeypatch):
    monkeypatch.setenv("MOJO_HIP_VALIDATE", "1")
    with pytest.raises(ValueError, match="fewer keys"):
        on_gpu(ops()[0], inputs([3, 40], 4))
    on_gpu(ops()[0], inputs([4, 40], 4))


def test_a_hole_row_is_the_single_step_op_step_by_step():
    """Negative page ids with no window: zero K/V from the first hole on, as in `HIPPagedDecodeGQAWithKVDequant`."""
    steps = 4
    q, _, k8, ks, v8, vs, lens, table = inputs([300, 70, 33], steps)
    table[0, 5] = -1
    table[1, 2] = -1
    got = on_gpu(ops("ABAB")[0], (q, None, k8, ks, v8, vs, lens, table))
    assert last_launch().endswith(":kv8:nstep")
    single = hip_cls("MojoPagedDecodeGQAWithKVDequant")(gqa_layout="ABAB")
    for j in range(steps):
        want = on_gpu(single, (q[:, j].contiguous(), None, k8, ks, v8, vs, lens - (steps - 1 - j), table))
        assert bool(torch.isfinite(got[:, j].float()).all())
        torch.testing.assert_close(got[:, j].float(), want.float(), atol=ATOL, rtol=RTOL)


@pytest.mark.parametrize("layout", [("nhd", "dense"), ("hnd", "offset"), ("padded", "wide")], ids="-".join)
def test_strided_cache_and_table_layouts(layout):
    steps = 4
    q, _, k8, ks, v8, vs, lens, table = inputs([300, 47, 4, 0], steps)
    hidden = CL.poison_page([k8, v8], CL.spare_pages(k8.shape[0], table)[0])
    caches, tb = CL.lay_out_kv(k8, v8, layout[0]).to(DEV), CL.lay_out_table(table, layout[1], hidden).to(DEV)
    hip, ref = ops("AABB", 4, 100)
    kc, vc = caches.views
    got = hip.forward(q.to(DEV), None, kc, ks.to(DEV), vc, vs.to(DEV), lens.to(DEV), tb.views[0])
    torch.cuda.synchronize()
    assert last_launch().endswith(":kv8:nstep")
    compare(got, ref.forward(q, None, k8, ks, v8, vs, lens, table), "-".join(layout))


def test_graph_replay_with_new_lengths_leaves_padded_rows_untouched():
    steps = 4
    q, _, k8, ks, v8, vs, lens, table = (x if x is None else x.to(DEV) for x in inputs([300, 200, 130, 90], steps))
    hip, ref = ops("AABB", 4, 100)
    hip.forward(q, None, k8, ks, v8, vs, lens, table)                   # warm-up (library load, attributes)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            out = hip.forward(q, None, k8, ks, v8, vs, lens, table, max_total_seq_len=300)
    out.fill_(7.0)
    lens.copy_(torch.tensor([290, 0, 77, 0], dtype=torch.int32, device=DEV))
    graph.replay()
    torch.cuda.synchronize()
    want = ref.forward(q.cpu(), None, k8.cpu(), ks.cpu(), v8.cpu(), vs.cpu(), lens.cpu(), table.cpu())
    got = out.cpu()
    assert bool((got[1] == 7.0).all()) and bool((got[3] == 7.0).all())
    compare(got[[0, 2]], want[[0, 2]], "replay")


@pytest.mark.parametrize("scale_dtype", [torch.bfloat16, torch.float32], ids=str)
def test_scale_dtypes(scale_dtype):
    q, _, k8, ks, v8, vs, lens, table = inputs([130, 47, 4, 0], 4)
    ks, vs = ks.to(scale_dtype), vs.to(scale_dtype)
    hip, ref = ops("ABAB", 4, 20)
    got = on_gpu(hip, (q, None, k8, ks, v8, vs, lens, table))
    assert last_launch().endswith(":kv8:nstep")
    compare(got, ref.forward(q, None, k8, ks, v8, vs, lens, table), str(scale_dtype))


def test_a_zero_query_row_gives_the_uniform_average():
    """Scores of 0.0 for every visible key: step j is the plain mean of the values it sees."""
    steps = 3
    q, _, k8, ks, v8, vs, lens, table = inputs([50, 35], steps, hq=4, hkv=2, d=64)
    q = torch.zeros_like(q)
    hip, ref = ops("AABB")
    got = on_gpu(hip, (q, None, k8, ks, v8, vs, lens, table))
    assert last_launch().endswith(":kv8:nstep")
    want = ref.forward(q, None, k8, ks, v8, vs, lens, table)
    compare(got, want, "uniform")
    from oracle.paged import index_pages
    for b, n in enumerate(lens.tolist()):
        v = index_pages(v8, table[b], n).float() * vs.float().unsqueeze(1)               # [Hkv, n, D]
        for j in range(steps):
            mean = v[:, : n - (steps - 1 - j)].mean(dim=1)                                   # [Hkv, D]
            torch.testing.assert_close(to_cpu(got)[b, j].float(), mean.repeat_interleave(2, dim=0), atol=ATOL, rtol=RTOL)
