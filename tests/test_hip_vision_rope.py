"""GPU tests of the vision tower's rotary pair (`MojoApplyVisionRoPE2D`, `MojoVisionRotaryEmbedding2D`) through the C ABI.

The apply op is compared bit for bit with the CPU golden (tests/vision_tower_golden.py, pinned to the reference by
tests/test_vision_tower_golden.py).  The embedding's positions are pinned exactly (with ``rope_dim = 4`` the only frequency is
1.0, so the angle IS the position) and its cos / sin are held to what a faithfully rounded fp32 ``cosf`` may differ from torch's
CPU one, measured against fp64 of the golden's own fp32 angle."""
import math

import pytest
import torch

import vision_tower_golden as G
from conftest import load_golden
from hip_utils import DEV, hip_cls, last_launch, run_hip_case, to_cpu
from test_hip_sdpa import dev

pytestmark = pytest.mark.gpu
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
APPLY, EMBED = "MojoApplyVisionRoPE2D", "MojoVisionRotaryEmbedding2D"


def differing(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    return int((got.float() != want.float()).sum())


@pytest.mark.parametrize("case", [pytest.param(c, id=f"{i}-{c['op']}") for i, c in enumerate(load_golden("vision_tower"))
                                  if c["op"] == APPLY])
def test_apply_captured_vectors(case):
    got = to_cpu(run_hip_case(case))
    if case["args"][0].dtype == F32:
        for a, b in zip(got, case["out"]):
            torch.testing.assert_close(a, b, atol=1e-6, rtol=1e-6)
    else:
        assert [differing(a, b) for a, b in zip(got, case["out"])] == [0, 0]


def tables(g, tokens, dim, dtype=F32):
    angle = torch.rand(tokens, dim, generator=g) * 6.0 - 3.0
    return angle.cos().to(dtype), angle.sin().to(dtype)


DIMS = [2, 4, 12, 64, 72, 80, 128]


@pytest.mark.parametrize("strided", [False, True], ids=["contiguous", "fused-slices"])
@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("tokens,heads", [(1, (1, 1)), (3, (3, 2)), (257, (20, 20))])
def test_apply_is_the_golden_bit_for_bit(tokens, heads, dtype, strided):
    """0 differing elements for every D of DIMS; `fused-slices`: q and k are slices of one [T, Nq + Nk + Nk, D] buffer that starts
    one element into its storage, which breaks 16-byte (and 4-byte) alignment of every row."""
    hip, ref = hip_cls(APPLY)(), G.TorchApplyVisionRoPE2D()
    nq, nk = heads
    for d in DIMS:
        g = torch.Generator().manual_seed(tokens * 1000 + d)
        cos, sin = tables(g, tokens, d)
        if strided:
            flat = torch.randn(tokens * (nq + 2 * nk) * d + 1, generator=g).to(dtype)
            fused = flat[1:].view(tokens, nq + 2 * nk, d)
            q, k = fused[:, :nq], fused[:, nq:nq + nk]
            assert q.data_ptr() % 4 != 0 and (tokens == 1 or not q.is_contiguous())
        else:
            q, k = torch.randn(tokens, nq, d, generator=g).to(dtype), torch.randn(tokens, nk, d, generator=g).to(dtype)
        want = ref.forward(q, k, cos, sin)
        got = to_cpu(hip.forward(dev(q), dev(k), cos.to(DEV), sin.to(DEV)))
        assert [differing(a, b) for a, b in zip(got, want)] == [0, 0], f"D={d}"
        assert got[0].is_contiguous() and got[1].is_contiguous()


def test_apply_vector_width_follows_half_of_d():
    """D = 72 has halves of 36 elements: 8-byte vectors; D = 80 takes 16-byte ones (both 16-bit; the launch is visible in the
    result only through its bits, which the test above pins: here the 16-bit tables, widened as the golden's promotion does)."""
    hip, ref = hip_cls(APPLY)(), G.TorchApplyVisionRoPE2D()
    g = torch.Generator().manual_seed(5)
    for d in (72, 80):
        for tdtype in (BF16, F16):
            q, k = torch.randn(9, 4, d, generator=g).to(BF16), torch.randn(9, 2, d, generator=g).to(BF16)
            cos, sin = tables(g, 9, d, tdtype)
            want = ref.forward(q, k, cos, sin)
            got = to_cpu(hip.forward(q.to(DEV), k.to(DEV), cos.to(DEV), sin.to(DEV)))
            assert [differing(a, b) for a, b in zip(got, want)] == [0, 0]


def test_apply_fp32_inputs():
    """fp32 inputs are bit-identical to the CPU golden as well: 0 of 2 x 257 x (3 + 2) x {64, 72, 128} elements differ (measured
    on MI355X; the golden's products and sum are separate torch calls, so no host can contract them).  The formula's own
    rounding bound against fp64 — two rounded products and a rounded sum, 3 * 2^-24 relative to |x cos| + |rot(x) sin| — is
    asserted beside it."""
    hip, ref = hip_cls(APPLY)(), G.TorchApplyVisionRoPE2D()
    g = torch.Generator().manual_seed(6)
    for d in (64, 72, 128):
        q, k = torch.randn(257, 3, d, generator=g), torch.randn(257, 2, d, generator=g)
        cos, sin = tables(g, 257, d)
        want = ref.forward(q, k, cos, sin)
        got = to_cpu(hip.forward(q.to(DEV), k.to(DEV), cos.to(DEV), sin.to(DEV)))
        for x, a, b in zip((q, k), got, want):
            print(f"fp32 D={d}: {differing(a, b)} of {a.numel()} elements differ from the CPU golden")
            assert differing(a, b) == 0
            exact = G.apply_vision_rope_fp64(x, cos, sin)
            half = d // 2
            rot = torch.cat((x[..., half:], x[..., :half]), dim=-1).double().abs()
            bound = 3 * 2.0 ** -24 * (x.double().abs() * cos.double().abs().unsqueeze(1) + rot * sin.double().abs().unsqueeze(1))
            assert bool(((a.double() - exact).abs() <= bound + 1e-45).all())


@pytest.mark.parametrize("pool,grids", [(1, [(4, 6)]), (2, [(4, 6)]), (2, [(8, 2)]), (4, [(8, 4)]), (2, [(4, 6), (8, 2), (2, 2)]),
                                        (1, [(3, 5), (1, 1), (7, 2)]), (4, [(4, 8), (8, 4), (4, 4)])])
def test_embedding_names_the_position_of_every_token(pool, grids):
    """rope_dim = 4: inv_freq = [1.0], the row is [h, w, h, w] as angles, so (cos, sin) of every token must be those of the
    (h, w) the definition gives (tests/vision_tower_golden.py::vision_positions) — compared through atan2, which recovers an
    integer angle below pi exactly enough to round, and directly against cos / sin of the integer."""
    hip = hip_cls(EMBED)(rope_theta=10000.0, rope_dim=4, adapooling_factor=pool).to(DEV)
    assert hip.inv_freq.tolist() == [1.0]
    cos, sin = hip.forward(torch.tensor(grids, dtype=torch.int32, device=DEV))
    cos, sin = to_cpu(cos), to_cpu(sin)
    pos = G.vision_positions(grids, pool)
    assert cos.shape == sin.shape == (pos.shape[0], 4) and cos.dtype == sin.dtype == F32
    want = torch.cat([pos, pos], dim=-1).double()
    assert float((cos.double() - want.cos()).abs().max()) <= 2e-7 and float((sin.double() - want.sin()).abs().max()) <= 2e-7
    # positions below 2 pi are recovered outright (grids of up to 6 rows / columns): the angle itself, to the integer
    small = want < 6.2
    angle = torch.atan2(sin.double(), cos.double()) % (2 * math.pi)
    assert torch.equal(angle[small].round(), want[small])
    assert last_launch() == f"vision_rotary_2d:pool{pool}"


@pytest.mark.parametrize("rope_dim", [64, 128])
def test_embedding_accuracy_on_the_references_grids(rope_dim):
    """Against fp64 cos / sin of the golden's own fp32 angle.  Allowance: what torch's CPU fp32 result shows against that fp64 on
    the same angles (computed here) plus 2^-23, one fp32 ulp below 1.0 — the room another faithfully rounded cosf may take; the
    reference's 1e-5 is the ceiling.  Measured on MI355X: cos 4.1e-8 (torch's CPU 3.3e-8 at rope_dim 64, 3.6e-8 at 128), sin 2.8e-8
    to 4.5e-8 (torch's CPU 2.8e-8 to 3.2e-8); the test prints every maximum."""
    for grids, pool in (([(4, 4)], 1), ([(8, 6)], 1), ([(8, 8), (4, 6)], 1), ([(8, 6), (2, 4), (4, 4)], 2)):
        ref = G.TorchVisionRotaryEmbedding2D(rope_theta=10000.0, rope_dim=rope_dim, adapooling_factor=pool)
        hip = hip_cls(EMBED)(rope_theta=10000.0, rope_dim=rope_dim, adapooling_factor=pool).to(DEV)
        grid = torch.tensor(grids, dtype=torch.int32)
        angle = ref.angles(grid)
        want_c, want_s = ref.forward(grid)
        cos, sin = hip.forward(grid)                           # a CPU grid is accepted: it is read on the host anyway
        cos, sin = to_cpu(cos), to_cpu(sin)
        for name, got, cpu, exact in (("cos", cos, want_c, angle.double().cos()), ("sin", sin, want_s, angle.double().sin())):
            torch_err = float((cpu.double() - exact).abs().max())
            err = float((got.double() - exact).abs().max())
            print(f"rope_dim {rope_dim} grids {grids} pool {pool} {name}: device {err:.3e}, torch CPU {torch_err:.3e}")
            assert err <= min(torch_err + 2.0 ** -23, 1e-5)
        # the duplicated halves are the same bits
        half = rope_dim // 2
        assert torch.equal(cos[:, :half], cos[:, half:]) and torch.equal(sin[:, :half], sin[:, half:])


def test_embedding_captured_vectors():
    for case in load_golden("vision_tower"):
        if case["op"] != EMBED:
            continue
        cos, sin = to_cpu(run_hip_case(case))
        for got, want in zip((cos, sin), case["out"]):
            assert got.shape == want.shape and got.dtype == want.dtype
            torch.testing.assert_close(got, want, atol=1e-5, rtol=1e-6)      # the reference's own tolerance
