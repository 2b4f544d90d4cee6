"""GPU tests of the multimodal RoPE (`MojoMRoPE`, `MojoMRoPEInplace`) through the C ABI.

With fp32 tables the in-place form is compared bit for bit with the CPU golden of ``MojoMRoPEInplace(inplace=True)`` and the
out-of-place form with the fp32 golden rounded once (tests/vision_tower_golden.py, pinned to the reference by
tests/test_vision_tower_golden.py).  The table every index takes is pinned exactly with tables of (1, 0), (0, 1) and (-1, 0)."""
import pytest
import torch

import vision_tower_golden as G
from conftest import load_golden
from dit_block_golden import ulp_distance
from hip_utils import DEV, hip_cls, last_launch, to_cpu

pytestmark = pytest.mark.gpu
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32


def inputs(g, tokens, hq, hk, hd, half, dtype, tdtype=F32, three=True):
    q = torch.randn(tokens, hq * hd, generator=g).to(dtype)
    k = torch.randn(tokens, hk * hd, generator=g).to(dtype)
    angle = torch.rand(*((3, tokens, half) if three else (tokens, half)), generator=g) * 6.0 - 3.0
    return q, k, angle.cos().to(tdtype), angle.sin().to(tdtype)


def differing(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    return int((got.float() != want.float()).sum())


def run_both(q, k, cos, sin, sec, inter, hd):
    """(in-place result, out-of-place result, inputs untouched by the out-of-place call) on the device, back on the CPU."""
    dq, dk, dc, ds = q.to(DEV), k.to(DEV), cos.to(DEV), sin.to(DEV)
    out = hip_cls("MojoMRoPE")().forward(dq, dk, dc, ds, sec, inter, hd)
    assert last_launch().startswith("mrope:") and ":copy:" in last_launch()
    untouched = torch.equal(dq.cpu(), q) and torch.equal(dk.cpu(), k) and out[0].data_ptr() != dq.data_ptr()
    again = hip_cls("MojoMRoPEInplace")(inplace=False).forward(dq, dk, dc, ds, sec, inter, hd)
    assert torch.equal(again[0], out[0]) and torch.equal(again[1], out[1]) and torch.equal(dq.cpu(), q)
    ret = hip_cls("MojoMRoPEInplace")(inplace=True).forward(dq, dk, dc, ds, sec, inter, hd)
    assert ":inplace:" in last_launch() and ret[0] is dq and ret[1] is dk
    return to_cpu((dq, dk)), to_cpu(out), untouched


MODEL_ROWS = [(28, 4, [16, 24, 24], False), (40, 8, [16, 24, 24], False), (16, 8, [24, 20, 20], True), (32, 8, [24, 20, 20], True)]
CASES = ([(t, hq, hk, 128, sec, inter) for hq, hk, sec, inter in MODEL_ROWS for t in (1, 32)] +
         [(5, 4, 2, 128, [8, 12, 12], False), (5, 4, 2, 128, [12, 18, 18], True), (5, 4, 2, 96, [8, 12, 12], True),   # partial / full
          (3, 3, 1, 8, [1, 1, 2], False), (3, 3, 1, 8, [1, 1, 2], True), (3, 2, 2, 12, [1, 1, 2], False), (3, 2, 2, 12, [1, 1, 2], True)])


@pytest.mark.parametrize("three", [True, False], ids=["tables3d", "tables2d"])
@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("tokens,hq,hk,hd,sec,inter", CASES)
def test_bit_exact_with_fp32_tables(tokens, hq, hk, hd, sec, inter, dtype, three):
    g = torch.Generator().manual_seed(tokens * 100 + hq + hd + sum(sec))
    q, k, cos, sin = inputs(g, tokens, hq, hk, hd, sum(sec), dtype, three=three)
    want_in = G.TorchMRoPEInplace(inplace=True).forward(q.clone(), k.clone(), cos, sin, sec, inter, hd)
    want_out = G.TorchMRoPE().forward(q, k, cos, sin, sec, inter, hd)
    assert want_out[0].dtype == F32                      # the reference's out-of-place result: torch's promotion
    got_in, got_out, untouched = run_both(q, k, cos, sin, sec, inter, hd)
    assert untouched
    assert [differing(a, b) for a, b in zip(got_in, want_in)] == [0, 0]
    assert [differing(a, b.to(dtype)) for a, b in zip(got_out, want_out)] == [0, 0]


def test_captured_vectors():
    for case in load_golden("vision_tower"):
        if not case["op"].startswith("MojoMRoPE"):
            continue
        q, k, cos, sin, sec, inter, hd = case["args"]
        op = hip_cls(case["op"])(**case["ctor"]["kwargs"])
        got = to_cpu(op.forward(q.to(DEV), k.to(DEV), cos.to(DEV), sin.to(DEV), sec, inter, hd))
        for a, b in zip(got, case["out"]):
            if cos.dtype == F32 and q.dtype != F32:
                assert differing(a, b.to(q.dtype)) == 0
            else:                                            # 16-bit tables, fp32 queries: the reference's tolerance
                torch.testing.assert_close(a.float(), b.float(), atol=3e-2 if q.dtype != F32 else 1e-5, rtol=6e-3 if q.dtype != F32 else 1e-5)


@pytest.mark.parametrize("dtype", [BF16, F16, F32], ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("inter", [False, True], ids=["chunked", "interleaved"])
@pytest.mark.parametrize("sec,hd", [([24, 20, 20], 128), ([2, 1, 3], 16), ([16, 24, 24], 128), ([1, 1, 2], 12), ([3, 0, 2], 10)])
def test_the_table_every_index_takes(sec, hd, inter, dtype):
    """Table 0 is (cos, sin) = (1, 0), table 1 (0, 1), table 2 (-1, 0): the output pair of half-index i is then exactly
    (h1, h2), (-h2, h1) or (-h1, -h2), in every dtype, which names the table the index took.  Elements past rope_dim are the
    input's bits."""
    half, tokens, heads = sum(sec), 4, 3
    g = torch.Generator().manual_seed(half + hd)
    x = torch.randn(tokens, heads * hd, generator=g).to(dtype)
    x = torch.where(x == 0, torch.ones_like(x), x)           # (no zero: every sign flip must show)
    y = torch.randn(tokens, 1 * hd, generator=g).to(dtype)
    y = torch.where(y == 0, torch.ones_like(y), y)
    cos = torch.tensor([1.0, 0.0, -1.0])[:, None, None].expand(3, tokens, half).contiguous()
    sin = torch.tensor([0.0, 1.0, 0.0])[:, None, None].expand(3, tokens, half).contiguous()
    table = torch.tensor(G.mrope_table_of(half, sec, inter))
    got_in, got_out, _ = run_both(x, y, cos, sin, sec, inter, hd)
    for src, results in ((x, (got_in[0], got_out[0])), (y, (got_in[1], got_out[1]))):
        h = src.view(tokens, -1, hd)
        h1, h2, rest = h[..., :half], h[..., half:2 * half], h[..., 2 * half:]
        first = torch.where(table == 0, h1, torch.where(table == 1, -h2, -h1))
        second = torch.where(table == 0, h2, torch.where(table == 1, h1, -h2))
        want = torch.cat([first, second, rest], dim=-1).view(tokens, -1)
        for got in results:
            assert got.dtype == dtype and torch.equal(got.view(torch.int16 if dtype != F32 else torch.int32),
                                                      want.contiguous().view(torch.int16 if dtype != F32 else torch.int32))


def test_in_place_on_slices_of_a_fused_qkv_row():
    """Only the rotated elements of q and k change: the pass-through tails, the v slice and a guard band around the buffer
    keep their bits."""
    g = torch.Generator().manual_seed(8)
    tokens, hq, hk, hd, sec, dtype = 7, 4, 2, 64, [8, 12, 8], BF16          # rope_dim 56: a tail of 8 per head
    half = sum(sec)
    width, guard = (hq + 2 * hk) * hd, 24
    whole = torch.randn(guard + tokens * width + guard, generator=g).to(dtype)
    before = whole.clone()
    d_whole = whole.to(DEV)
    rows = d_whole[guard:guard + tokens * width].view(tokens, width)
    dq, dk = rows[:, :hq * hd], rows[:, hq * hd:(hq + hk) * hd]
    assert not dq.is_contiguous() and dq.stride(0) == width
    _, _, cos, sin = inputs(g, tokens, hq, hk, hd, half, dtype)
    ret = hip_cls("MojoMRoPEInplace")(inplace=True).forward(dq, dk, cos.to(DEV), sin.to(DEV), sec, True, hd)
    torch.cuda.synchronize()
    assert ret[0] is dq and ret[1] is dk
    after = d_whole.cpu()
    host_rows = before[guard:guard + tokens * width].view(tokens, width)
    want_q, want_k = G.TorchMRoPEInplace(inplace=True).forward(host_rows[:, :hq * hd].clone(), host_rows[:, hq * hd:(hq + hk) * hd].clone(),
                                                               cos, sin, sec, True, hd)
    want = before.clone()
    want_rows = want[guard:guard + tokens * width].view(tokens, width)
    want_rows[:, :hq * hd], want_rows[:, hq * hd:(hq + hk) * hd] = want_q, want_k
    assert torch.equal(after.view(torch.int16), want.view(torch.int16))
    changed = (after.view(torch.int16) != before.view(torch.int16)).nonzero().flatten()
    inside = (changed - guard) % width
    assert bool(((changed >= guard) & (changed < guard + tokens * width) & (inside < (hq + hk) * hd) & (inside % hd < 2 * half)).all())
    # the out-of-place call on the same slices reads them in place and gives the same bits
    d_again = before.to(DEV)
    rows2 = d_again[guard:guard + tokens * width].view(tokens, width)
    out = hip_cls("MojoMRoPE")().forward(rows2[:, :hq * hd], rows2[:, hq * hd:(hq + hk) * hd], cos.to(DEV), sin.to(DEV), sec, True, hd)
    assert torch.equal(out[0].cpu(), want_q) and torch.equal(out[1].cpu(), want_k) and torch.equal(d_again.cpu(), before)


@pytest.mark.parametrize("hd,sec", [(128, [16, 24, 24]), (72, [8, 12, 12]), (12, [1, 1, 2])])
def test_fp32_queries(hd, sec):
    """fp32 queries are bit-identical to the CPU golden as well: 0 differing elements on every case here (measured on MI355X;
    the golden's products, difference and sum are separate torch calls, so no host can contract them).  The formula's own
    rounding bound against fp64, 3 * 2^-24 relative to |h1 c| + |h2 s|, is asserted beside it."""
    g = torch.Generator().manual_seed(hd)
    for inter in (False, True):
        q, k, cos, sin = inputs(g, 33, 3, 2, hd, sum(sec), F32)
        want = G.TorchMRoPE().forward(q, k, cos, sin, sec, inter, hd)
        got_in, got_out, _ = run_both(q, k, cos, sin, sec, inter, hd)
        for x, a, b, w in zip((q, k), got_in, got_out, want):
            assert torch.equal(a, b)
            print(f"fp32 hd={hd} inter={inter}: {differing(a, w)} of {a.numel()} elements differ from the CPU golden")
            assert differing(a, w) == 0
            exact = G.mrope_fp64(x, cos, sin, sec, inter, hd)
            zero = torch.zeros_like(cos)                     # |h1 c| + |h2 s| and |h2 c| + |h1 s|, from the two halves of the formula
            mag = G.mrope_fp64(x.abs(), cos.abs(), zero, sec, inter, hd) + G.mrope_fp64(x.abs(), zero, sin.abs(), sec, inter, hd).abs()
            assert bool(((a.double() - exact).abs() <= 3 * 2.0 ** -24 * mag + 1e-45).all())


@pytest.mark.parametrize("tdtype", [BF16, F16], ids=["bf16-tables", "fp16-tables"])
@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "fp16"])
def test_16_bit_tables_are_within_one_storage_ulp_of_fp64(dtype, tdtype):
    """The tables are converted on read and the math is fp32, so the result is the fp64 formula on the stored values to one
    storage ulp (the golden computes in the 16-bit type and rounds three times); the reference's atol 3e-2 / rtol 6e-3 is the
    ceiling."""
    g = torch.Generator().manual_seed(3)
    for hd, sec, inter in ((128, [16, 24, 24], False), (128, [24, 20, 20], True), (96, [8, 12, 12], True)):
        q, k, cos, sin = inputs(g, 17, 4, 2, hd, sum(sec), dtype, tdtype)
        got_in, got_out, _ = run_both(q, k, cos, sin, sec, inter, hd)
        ref = G.TorchMRoPE().forward(q, k, cos, sin, sec, inter, hd)
        for x, a, b, r in zip((q, k), got_in, got_out, ref):
            assert torch.equal(a, b)
            exact = G.mrope_fp64(x, cos, sin, sec, inter, hd)
            assert int(ulp_distance(a, exact).max()) <= 1
            torch.testing.assert_close(a.float(), r.float(), atol=3e-2, rtol=6e-3)


def test_validation_errors_name_the_argument():
    q, k = torch.zeros(3, 64, dtype=BF16, device=DEV), torch.zeros(3, 32, dtype=BF16, device=DEV)
    tab = torch.zeros(3, 3, 8, device=DEV)
    for op in (hip_cls("MojoMRoPE")(), hip_cls("MojoMRoPEInplace")(inplace=True)):
        with pytest.raises(ValueError, match="mrope_section"):
            op.forward(q, k, tab, tab, [4, 4], False, 16)
        with pytest.raises(ValueError, match="more than head_dim"):
            op.forward(q, k, tab, tab, [4, 2, 2], False, 12)
        with pytest.raises(ValueError, match="query row width"):
            op.forward(q[:, :60], k, tab, tab, [2, 3, 3], False, 16)
        with pytest.raises(ValueError, match="key row width"):
            op.forward(q, k[:, :30], tab, tab, [2, 3, 3], False, 16)
        with pytest.raises(ValueError, match="token counts"):
            op.forward(q, k[:2], tab, tab, [2, 3, 3], False, 16)
        with pytest.raises(ValueError, match="cos_table of shape"):
            op.forward(q, k, tab[:, :, :4], tab[:, :, :4], [2, 3, 3], False, 16)
    assert not bool(q.any()) and not bool(k.any())
