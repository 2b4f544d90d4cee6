"""GPU parity of the bidirectional attention with an optional mask (`MojoSdpa`) through the C ABI.

Tolerance: atol = rtol = 2e-2 over every element, the project's attention bound.  The oracle is tests/sdpa_golden.py on the CPU
(pinned to the reference by tests/test_sdpa_golden.py).  Sizes sit around the kernel's edges: the key tile is 64 keys and a
workgroup owns 128 / G query positions.  Every random boolean mask keeps one key visible per row, so no row torch leaves
undefined enters a tolerance comparison; rows with no visible key are checked apart (exact zeros: beyond the reference).

Every case runs in three launch forms — unsplit, the key split forced (MOJO_HIP_PREFILL_KSPLIT) and general staging
(MOJO_HIP_PREFILL_FAST_STAGE=0) — and `mojo_hip_last_launch()` is asserted each time."""
import pytest
import torch

import sdpa_golden
import visibility_sdpa as vis
from conftest import load_golden
from hip_utils import DEV, assert_close_tree, hip_cls, last_launch, run_hip_case, switch_env, to_cpu

pytestmark = pytest.mark.gpu
ATOL = RTOL = 2e-2
NAME = "MojoSdpa"
# (switches, stage tag, ksplit tag).  A forced split of 3 cuts a block of >= 24 key tiles three ways; shorter blocks keep one
# live slice and the merge launch still runs.
FORMS = [(dict(MOJO_HIP_PREFILL_KSPLIT="1", MOJO_HIP_PREFILL_FAST_STAGE=None), "fast_stage", 1),
         (dict(MOJO_HIP_PREFILL_KSPLIT="3", MOJO_HIP_PREFILL_FAST_STAGE=None), "fast_stage", 3),
         (dict(MOJO_HIP_PREFILL_KSPLIT="1", MOJO_HIP_PREFILL_FAST_STAGE="0"), "general_stage", 1)]


def ops(scale=None, gqa=True):
    return hip_cls(NAME)(scale=scale, enable_gqa=gqa), sdpa_golden.TorchSdpa(scale=scale, enable_gqa=gqa)


def dev(t):
    """The tensor on the device WITH its strides (views stay views of one buffer)."""
    if t is None:
        return None
    flat = torch.empty(0, dtype=t.dtype).set_(t.untyped_storage(), 0, (t.untyped_storage().nbytes() // t.element_size(),), (1,))
    return torch.as_strided(flat.to(DEV), t.shape, t.stride(), t.storage_offset())


def on_gpu(op, q, k, v, mask=None):
    out = op.forward(dev(q), dev(k), dev(v), dev(mask))
    torch.cuda.synchronize()
    return out


def expect_tag(stage, ksplit, masked):
    want = f"sdpa:default:{stage}:ksplit{ksplit}" + (":mask" if masked else "")
    assert last_launch() == want, (last_launch(), want)


def in_every_form(hip, q, k, v, mask, want):
    """Run the call in the three launch forms; each is within tolerance of ``want`` (CPU).  Returns the outputs."""
    outs = []
    for env, stage, ksplit in FORMS:
        with switch_env(**env):
            got = on_gpu(hip, q, k, v, mask)
            expect_tag(stage, ksplit, mask is not None)
        outs.append(to_cpu(got))
        assert_close_tree(outs[-1], want, ATOL, RTOL)
    return outs


def qkv(g, b, hq, hkv, sq, sk, d, dtype, token_major=False):
    def one(h, s):
        if token_major:                                    # [B,S,H,D] memory seen as [B,H,S,D]
            return torch.randn(b, s, h, d, generator=g).to(dtype).transpose(1, 2)
        return torch.randn(b, h, s, d, generator=g).to(dtype)
    return one(hq, sq), one(hkv, sk), one(hkv, sk)


def random_bool(g, shape, p=0.5):
    m = torch.rand(shape, generator=g) < p
    m[..., int(torch.randint(0, shape[-1], (1,), generator=g))] = True   # one visible key in every row
    return m


@pytest.mark.parametrize("case", [pytest.param(c, id=f"{i}-{c['mask_form']}") for i, c in enumerate(load_golden("sdpa"))])
def test_captured_vectors(case):
    assert_close_tree(to_cpu(run_hip_case(case)), case["out"], ATOL, RTOL)
    assert last_launch().startswith("sdpa:default:") and last_launch().endswith(":mask") == (case["args"][3] is not None)


# Sq around the query block (128 / G rows), Sk around the key tile (64); Sq > Sk, Sq == Sk and Sq < Sk all occur
SKS = [1, 63, 64, 65, 130, 257]
DIMS = [64, 96, 128]


def _parity_cases():
    cases, i = [], 0
    for G in (1, 2, 4, 8):
        for sq in (1, 17, 128 // G - 1, 128 // G + 1, 200):
            sk = SKS[i % len(SKS)]
            cases.append(pytest.param(G, sq, sk, DIMS[i % 3], (1, 3)[i % 2], (torch.bfloat16, torch.float16)[(i // 2) % 2],
                                      (None, 0.3)[(i // 3) % 2], id=f"G{G}-Sq{sq}-Sk{sk}-D{DIMS[i % 3]}-B{(1, 3)[i % 2]}"))
            i += 1
    cases += [pytest.param(1, 64, 64, 128, 1, torch.bfloat16, None, id="G1-Sq64-Sk64-equal"),
              pytest.param(4, 33, 33, 64, 3, torch.float16, None, id="G4-Sq33-Sk33-equal"),
              pytest.param(2, 70, 1700, 128, 1, torch.bfloat16, None, id="G2-Sq70-Sk1700-split3"),
              pytest.param(8, 20, 1537, 64, 1, torch.float16, 0.2, id="G8-Sq20-Sk1537-split3")]
    return cases


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "boolmask"])
@pytest.mark.parametrize("G,sq,sk,d,b,dtype,scale", _parity_cases())
def test_parity_around_the_tile_and_block_edges(G, sq, sk, d, b, dtype, scale, masked):
    g = torch.Generator().manual_seed(1000 * G + sq + sk)
    hkv = 2 if G < 8 else 1
    q, k, v = qkv(g, b, hkv * G, hkv, sq, sk, d, dtype)
    mask = random_bool(g, (b, hkv * G, sq, sk)) if masked else None
    hip, ref = ops(scale)
    in_every_form(hip, q, k, v, mask, ref.forward(q, k, v, mask))


def block_causal(sq, sk, block=32):
    return (torch.arange(sq)[:, None] // block) >= (torch.arange(sk)[None, :] // block)


MASK_FORMS = ["bool_2d", "bool_b1", "key_padding", "block", "bias", "bias_fp32", "bias_inf", "last_stride", "expanded"]


@pytest.mark.parametrize("sk", [65, 130, 256])
@pytest.mark.parametrize("form", MASK_FORMS)
def test_mask_forms(form, sk):
    b, hq, hkv, sq, d, dtype = 3, 4, 2, 50, 64, torch.bfloat16
    g = torch.Generator().manual_seed(sk + len(form))
    q, k, v = qkv(g, b, hq, hkv, sq, sk, d, dtype)
    scale = None
    if form == "bool_2d":
        mask = random_bool(g, (sq, sk))
    elif form == "bool_b1":
        mask = random_bool(g, (b, 1, sq, sk))
    elif form == "key_padding":                            # [B,1,1,Sk]: stride-0 rows
        mask = torch.arange(sk)[None, None, None, :] < torch.tensor([sk, sk // 2, 1])[:, None, None, None]
    elif form == "block":
        mask = block_causal(sq, sk)
    elif form in ("bias", "bias_fp32"):                    # T5: an additive position bias, scale 1
        mask, scale = torch.randn(1, hq, sq, sk, generator=g).to(dtype if form == "bias" else torch.float32), 1.0
        q = q * 0.2
    elif form == "bias_inf":
        mask = torch.randn(1, hq, sq, sk, generator=g).to(dtype).masked_fill(~random_bool(g, (1, hq, sq, sk), 0.7), float("-inf"))
    elif form == "last_stride":                            # last stride 2: copied by the operator
        mask = random_bool(g, (b, 1, sq, 2 * sk))[..., ::2]
        mask[..., 0] = True
        assert mask.stride(-1) == 2
    else:                                                  # expanded by the caller: stride 0 over batch and heads, never copied
        mask = random_bool(g, (sq, sk)).expand(b, hq, sq, sk)
    hip, ref = ops(scale)
    in_every_form(hip, q, k, v, mask, ref.forward(q, k, v, mask))


@pytest.mark.parametrize("mdtype", ["query", "fp32"])
@pytest.mark.parametrize("sk,d,dtype", [(65, 64, torch.bfloat16), (256, 128, torch.float16), (1100, 96, torch.bfloat16)])
def test_exact_a_bool_mask_and_its_float_form_give_the_same_bits(sk, d, dtype, mdtype):
    g = torch.Generator().manual_seed(sk)
    q, k, v = qkv(g, 1, 4, 1, 37, sk, d, dtype)
    keep = random_bool(g, (1, 1, 37, sk))
    bias = torch.zeros(keep.shape, dtype=dtype if mdtype == "query" else torch.float32).masked_fill(~keep, float("-inf"))
    hip, _ = ops()
    for env, stage, ksplit in FORMS:
        with switch_env(**env):
            a = to_cpu(on_gpu(hip, q, k, v, keep))
            b = to_cpu(on_gpu(hip, q, k, v, bias))
            expect_tag(stage, ksplit, True)
        assert torch.equal(a, b)


@pytest.mark.parametrize("as_bias", [False, True], ids=["bool", "bias"])
def test_rows_with_no_visible_key_are_exact_zeros(as_bias):
    """Beyond the reference (torch: NaN).  The other rows of the call are within tolerance of the step-by-step attention."""
    g = torch.Generator().manual_seed(9)
    b, hq, hkv, sq, sk, d, dtype = 3, 4, 2, 70, 130, 128, torch.bfloat16
    q, k, v = qkv(g, b, hq, hkv, sq, sk, d, dtype)
    keep = random_bool(g, (b, 1, sq, sk))
    dead = torch.zeros(b, 1, sq, dtype=torch.bool)
    dead[0, 0, 0] = dead[1, 0, 33] = dead[2, 0, 69] = True
    dead[1, 0, 40:60] = True
    keep[dead] = False
    mask = torch.zeros(keep.shape, dtype=dtype).masked_fill(~keep, float("-inf")) if as_bias else keep
    want = sdpa_golden.reference_fp32(q, k, v, mask, enable_gqa=True).to(dtype)
    hip, _ = ops()
    for got in in_every_form(hip, q, k, v, mask, want):
        rows = dead[:, 0][:, None, :].expand(b, hq, sq)
        assert not bool(got[rows].any()) and bool(torch.isfinite(got.float()).all())


def test_layouts_are_read_and_written_in_place():
    g = torch.Generator().manual_seed(21)
    b, hq, hkv, sq, sk, d, dtype = 3, 4, 2, 45, 100, 128, torch.bfloat16
    hip, ref = ops()
    # the token-major view Wan passes: x.view(b, s, n, d).transpose(1, 2); the output has the same form
    q, k, v = qkv(g, b, hq, hkv, sq, sk, d, dtype, token_major=True)
    want = ref.forward(q, k, v)
    got = on_gpu(hip, q, k, v)
    assert got.shape == q.shape and got.stride() == q.stride()
    assert_close_tree(to_cpu(got), want, ATOL, RTOL)
    # contiguous [B,H,S,D]
    qc = q.contiguous()
    got_c = on_gpu(hip, qc, k.contiguous(), v.contiguous())
    assert got_c.is_contiguous() and torch.equal(to_cpu(got_c), to_cpu(got))
    # K/V as views of ONE fused buffer [B,S,(Hq + 2 Hkv),D]
    fused = torch.randn(b, sk, hq + 2 * hkv, d, generator=g).to(dtype)
    kf, vf = fused[:, :, hq:hq + hkv].transpose(1, 2), fused[:, :, hq + hkv:].transpose(1, 2)
    assert kf.stride() == vf.stride() and not kf.is_contiguous()
    assert_close_tree(to_cpu(on_gpu(hip, qc, kf, vf)), ref.forward(qc, kf, vf), ATOL, RTOL)
    # a misaligned K (base 2 bytes off a 16-byte boundary): copied
    pad = torch.randn(b * hkv * sk * d + 1, generator=g).to(dtype)
    km = pad[1:].view(b, hkv, sk, d)
    got_m = on_gpu(hip, qc, km, v.contiguous())
    assert_close_tree(to_cpu(got_m), ref.forward(qc, km, v), ATOL, RTOL)
    # 3-D input: one batch entry
    got3 = on_gpu(hip, qc[0], kf[0], vf[0])
    assert got3.shape == qc[0].shape
    assert_close_tree(to_cpu(got3), ref.forward(qc[0], kf[0], vf[0]), ATOL, RTOL)
    # no key at all: zeros (beyond the reference)
    assert not bool(to_cpu(on_gpu(hip, qc, km[:, :, :0], km[:, :, :0])).any())


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("G,sq,sk,d,dtype", [(1, 130, 65, 64, torch.bfloat16), (4, 33, 257, 128, torch.float16),
                                             (8, 17, 64, 96, torch.bfloat16), (2, 5, 1600, 128, torch.bfloat16)])
def test_exact_visible_set(G, sq, sk, d, dtype, masked):
    """Key by key: an invisible probe reads exactly 0, a visible one storage(fp32(1 / n)) within 1 ulp; rows past Sk and the
    gap between batch entries hold poison (tests/visibility_sdpa.py)."""
    b, hkv = 3, 2
    q, kbuf, vbuf, keys = vis.build(b, hkv * G, hkv, sq, sk, d, dtype)
    k, v = vis.views(kbuf, vbuf, sk)
    g = torch.Generator().manual_seed(sk)
    mask = random_bool(g, (b, hkv * G, sq, sk)) if masked else None
    visible = mask if masked else torch.ones(b, hkv * G, sq, sk, dtype=torch.bool)
    want, seen = vis.expected(visible, keys, dtype)
    hip, _ = ops(scale=1.0)
    for env, stage, ksplit in FORMS:
        with switch_env(**env):
            got = on_gpu(hip, q, k, v, mask)
            expect_tag(stage, ksplit, masked)
        vis.compare(to_cpu(got), want, seen)


def test_bits_are_identical_run_to_run_and_a_captured_call_replays_them():
    g = torch.Generator().manual_seed(4)
    q, k, v = qkv(g, 1, 8, 2, 150, 1700, 128, torch.bfloat16, token_major=True)
    mask = random_bool(g, (1, 1, 150, 1700))
    hip, _ = ops()
    dq, dk, dv, dm = dev(q), dev(k), dev(v), dev(mask)
    for env, stage, ksplit in FORMS:
        with switch_env(**env):
            for m in (None, dm):
                first = hip.forward(dq, dk, dv, m)
                again = hip.forward(dq, dk, dv, m)
                torch.cuda.synchronize()
                expect_tag(stage, ksplit, m is not None)
                assert torch.equal(first, again)
    # one call captured in a graph replays the eager bits (no host sync in the operator)
    eager = hip.forward(dq, dk, dv, dm)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        hip.forward(dq, dk, dv, dm)                          # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = hip.forward(dq, dk, dv, dm)
    captured.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured, eager)
