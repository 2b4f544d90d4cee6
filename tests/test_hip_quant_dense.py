"""GPU parity of the dense W8A8 quantiser ops (`QUANT_DENSE_OPS`) through the C ABI.

Bounds.  `MojoStaticQuant` and `MojoDequant` are single IEEE operations per element: `torch.equal` with the golden.  The
norm+quant ops and `MojoDequantSwiGLUQuant` take the project's norm+quant criterion (tests/test_hip_quantizers.py
`_check_norm_quant`): scale within rtol 1e-5, q within one step (fp8: 32), at most 2e-3 of the elements differing, the returned
residual `torch.equal`.  The norms differ from the golden through the fp32 row statistics (summation order), the SwiGLU stage
through the device library's expf; either can move a value that sits on a rounding boundary by one step.
tests/test_quant_dense_golden.py shows on the CPU that the inputs used here leave room for that bound.

Launch tags (`last_launch()`):
  rmsnorm_quant:wide|scalar:tpr256:cached|nt          MojoRMSNormQuant (norm_quant_kernel, no residual)
  layernorm_quant:wide|scalar:resident|reread:cached|nt   the two LayerNorm ops
  static_quant:wide|scalar:cached|nt                  MojoStaticQuant
  dequant:trailing|token:wide|scalar:cached|nt        MojoDequant
  dequant_swiglu_quant:wide|scalar:resident|reread:cached|nt
(the scalar forms have no non-temporal twin and always say `cached`)
"""
import pytest
import torch

import quant_dense_utils as U
from conftest import bit_equal, load_golden
from hip_utils import DEV, hip_cls, last_launch, run_hip_case, switch_env, to_cpu, torch_cls
from quant_dense_utils import BF16, F16, F32, F8, I8

pytestmark = pytest.mark.gpu

CASES = load_golden("quant_dense")
QUANT_KINDS = [(I8, True), (I8, False), (F8, True)]           # (quant dtype, symmetric)


def check_quant(q, scale, want_q, want_scale, quant_dtype, what=""):
    """The project's norm+quant criterion on (q, scale); returns the number of differing elements."""
    assert q.dtype == quant_dtype and q.shape == want_q.shape and scale.dtype == F32 and scale.shape == want_scale.shape, what
    torch.testing.assert_close(scale, want_scale, atol=0, rtol=1e-5)
    diff = (q.float() - want_q.float()).abs()
    step = 1.0 if quant_dtype == I8 else 32.0                 # fp8: integers up to 448 are spaced by up to 32
    share = float((diff > 0).float().mean())
    print(f"{what}: {int((diff > 0).sum())} of {diff.numel()} quantised values differ (share {share:.2e}, largest {float(diff.max())})")
    assert float(diff.max()) <= step, what
    assert share <= 2e-3, what
    return int((diff > 0).sum())


def misaligned(t, offset=1):
    """``t``'s values on the device in a contiguous view that starts ``offset`` elements into a fresh buffer."""
    flat = torch.empty(t.numel() + offset, dtype=t.dtype, device=DEV)
    view = flat[offset:].view(t.shape)
    view.copy_(t.to(DEV))                                     # device to device: a copy kernel, whatever the alignment
    assert bit_equal(view, t) and view.data_ptr() % 16 != 0
    return view


def both_policies(run, tag, has_nt=True):
    """``run()`` with MOJO_HIP_STREAM_NT=0, then =1: asserts the two tags and that the outputs are bit-identical; returns the
    cached run's outputs on the CPU."""
    with switch_env(MOJO_HIP_STREAM_NT="0"):
        cached = run()
        assert last_launch() == tag + ":cached", (last_launch(), tag)
    with switch_env(MOJO_HIP_STREAM_NT="1"):
        streamed = run()
        assert last_launch() == tag + (":nt" if has_nt else ":cached"), (last_launch(), tag)
    cached, streamed = to_cpu(cached), to_cpu(streamed)
    cached = cached if isinstance(cached, tuple) else (cached,)
    streamed = streamed if isinstance(streamed, tuple) else (streamed,)
    assert len(cached) == len(streamed) and all(bit_equal(a, b) for a, b in zip(cached, streamed)), tag
    return cached


def on_dev(*ts):
    return tuple(None if t is None else t.to(DEV) for t in ts)


# ---- fixtures through the C ABI ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [pytest.param(c, id=f"{c['op']}-{i}") for i, c in enumerate(CASES)])
def test_fixtures_through_the_c_abi(case):
    got, want, name = to_cpu(run_hip_case(case)), case["out"], case["op"]
    if name == "MojoDequant":
        assert got.dtype == want.dtype and torch.equal(got, want)
    elif name == "MojoStaticQuant":
        assert got[0].dtype == want[0].dtype and bit_equal(got[0], want[0]) and torch.equal(got[1], want[1])
    elif name == "MojoResidualAddLayerNormQuant":
        assert got[1].dtype == want[1].dtype and torch.equal(got[1], want[1])
        check_quant(got[0], got[2], want[0], want[2], case["ctor"]["kwargs"].get("quant_dtype", I8), name)
    else:
        check_quant(got[0], got[1], want[0], want[1], case["ctor"]["kwargs"].get("quant_dtype", I8), name)


# ---- the norm + quant ops: reference-space sweep ---------------------------------------------------------------------------
def norm_pair(name, dim, state, **kwargs):
    ref = U.make_op(U.golden_cls(name), state, norm_size=dim, **kwargs)
    op = U.make_op(hip_cls(name), state, device=DEV, norm_size=dim, **kwargs)
    return ref, op


@pytest.mark.parametrize("dtype", U.NORM_DTYPES, ids=str)
@pytest.mark.parametrize("shape", U.SWEEP_SHAPES, ids=str)
def test_norm_quant_reference_space(shape, dtype):
    x, r, w, b, smooth = U.norm_inputs(shape, dtype)
    dim = shape[-1]
    xd, rd, sd = on_dev(x, r, smooth)
    wide = dim % (16 // x.element_size()) == 0
    resident = dim // (16 // x.element_size() if wide else 1) <= (1024 if wide else 2048)
    ln_tag = f"layernorm_quant:{'wide' if wide else 'scalar'}:{'resident' if resident else 'reread'}:cached"
    with torch.no_grad():
        for quant_dtype, symmetric in QUANT_KINDS:
            kw = {"quant_dtype": quant_dtype, "symmetric": symmetric}
            for sm, smd in ((None, None), (smooth, sd)):
                what = f"{shape} {dtype} {quant_dtype} symmetric {symmetric} smooth {sm is not None}"
                ref, op = norm_pair("MojoRMSNormQuant", dim, {"weight": w}, **kw)
                want, got = ref(x, sm), to_cpu(op(xd, smd))
                assert last_launch() == f"rmsnorm_quant:{'wide' if wide else 'scalar'}:tpr256:cached", last_launch()
                check_quant(*got, *want, quant_dtype, "rmsnorm " + what)
                if quant_dtype == I8:                         # the reference's own acceptance call (test_normalization.py:463)
                    op.forward_diff_with(ref, xd, smd, atol=(1, 1e-3), rtol=(0, 1e-3), ref_device="cpu")
                ref, op = norm_pair("MojoLayerNormQuant", dim, {"weight": w, "bias": b}, **kw)
                want, got = ref(x, sm), to_cpu(op(xd, smd))
                assert last_launch() == ln_tag, last_launch()
                check_quant(*got, *want, quant_dtype, "layernorm " + what)
                if quant_dtype == I8:                         # (:492)
                    op.forward_diff_with(ref, xd, smd, atol=(1, 1e-3), rtol=(0, 1e-3), ref_device="cpu")
                for pos in ("pre", "post"):
                    ref, op = norm_pair("MojoResidualAddLayerNormQuant", dim, {"weight": w, "bias": b}, norm_pos=pos, **kw)
                    want, got = ref(x, r, sm), to_cpu(op(xd, rd, smd))
                    assert last_launch() == ln_tag, last_launch()
                    assert got[1].dtype == dtype and torch.equal(got[1], want[1])
                    check_quant(got[0], got[2], want[0], want[2], quant_dtype, f"add+layernorm {pos} " + what)
                    if quant_dtype == I8:                     # (:557)
                        op.forward_diff_with(ref, xd, rd, smd, atol=(1, 1e-3, 1e-3), rtol=(0, 1e-3, 1e-3), ref_device="cpu")
        if shape == (32, 1024):                               # elementwise_affine=False
            ref, op = norm_pair("MojoLayerNormQuant", dim, None, elementwise_affine=False)
            check_quant(*to_cpu(op(xd, sd)), *ref(x, smooth), I8, "layernorm, no affine")


@pytest.mark.parametrize("dtype", [F16, BF16], ids=str)
def test_norm_quant_non_contiguous_and_3d_inputs(dtype):
    x, r, w, b, smooth = U.norm_inputs((12, 1024), dtype)
    with torch.no_grad():
        for view in (lambda t: t[:, ::2], lambda t: t.view(3, 4, 1024), lambda t: t.view(2, 6, 1024)[:, 1:5]):
            xv, rv = view(x), view(r)
            dim = xv.shape[-1]
            xd, rd = view(x.to(DEV)), view(r.to(DEV))
            assert xd.is_contiguous() == xv.is_contiguous()
            ref, op = norm_pair("MojoRMSNormQuant", dim, {"weight": w[:dim]})
            got = to_cpu(op(xd))
            assert got[0].shape == xv.shape and got[1].shape == xv.shape[:-1] + (1,)
            check_quant(*got, *ref(xv), I8, "rmsnorm view")
            ref, op = norm_pair("MojoResidualAddLayerNormQuant", dim, {"weight": w[:dim], "bias": b[:dim]}, norm_pos="post")
            want, got = ref(xv, rv, smooth[:dim]), to_cpu(op(xd, rd, smooth[:dim].to(DEV)))
            assert torch.equal(got[1], want[1])
            check_quant(got[0], got[2], want[0], want[2], I8, "add+layernorm view")


# (rows, dim for the 16-bit types, tag)
NORM_FORMS = [(52, 1024, "wide:resident"), (52, 1001, "scalar:resident"), (7, 8200, "wide:reread"), (26, 2051, "scalar:reread"),
              (8195, 8, "wide:resident")]


@pytest.mark.parametrize("dtype", U.NORM_DTYPES, ids=str)
@pytest.mark.parametrize("form", NORM_FORMS, ids=lambda f: f"{f[2]}-{f[0]}x{f[1]}")
def test_norm_quant_launch_forms(form, dtype):
    """Every launch form of the LayerNorm kernel (and the tags of `MojoRMSNormQuant`) once, cached and non-temporal: the
    non-temporal twin gives the cached form's bits."""
    rows, dim, form_tag = form
    if dtype == F32 and form_tag.startswith("wide"):
        dim //= 2                                             # the same number of 16-byte vectors per row
    x, r, w, b, smooth = U.norm_inputs((rows, dim), dtype)
    xd, rd, sd = on_dev(x, r, smooth)
    has_nt = form_tag.startswith("wide")
    with torch.no_grad():
        for quant_dtype in (I8, F8):
            ref, op = norm_pair("MojoResidualAddLayerNormQuant", dim, {"weight": w, "bias": b}, quant_dtype=quant_dtype)
            want = ref(x, r, smooth)
            got = both_policies(lambda: op(xd, rd, sd), "layernorm_quant:" + form_tag, has_nt)
            assert torch.equal(got[1], want[1])
            check_quant(got[0], got[2], want[0], want[2], quant_dtype, f"add+layernorm {form_tag} {dtype}")
            ref, op = norm_pair("MojoLayerNormQuant", dim, {"weight": w, "bias": b}, quant_dtype=quant_dtype)
            got = both_policies(lambda: op(xd), "layernorm_quant:" + form_tag, has_nt)
            check_quant(*got, *ref(x), quant_dtype, f"layernorm {form_tag} {dtype}")
            ref, op = norm_pair("MojoRMSNormQuant", dim, {"weight": w}, quant_dtype=quant_dtype)
            got = both_policies(lambda: op(xd, sd), f"rmsnorm_quant:{form_tag.split(':')[0]}:tpr256", has_nt)
            check_quant(*got, *ref(x, smooth), quant_dtype, f"rmsnorm {form_tag} {dtype}")


# ---- static quant, dequant: bit-exact ----------------------------------------------------------------------------------------
def static_pair(scale, quant_dtype):
    state = {"scale": scale}
    kw = {"input_size": tuple(scale.shape), "quant_dtype": quant_dtype}
    return U.make_op(U.golden_cls("MojoStaticQuant"), state, **kw), U.make_op(hip_cls("MojoStaticQuant"), state, device=DEV, **kw)


def static_inputs(shape, scale_shape, dtype, quant_dtype):
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(shape, generator=g).to(dtype)
    scale = (torch.rand(scale_shape, generator=g) + 0.25) * (3.0 / (127 if quant_dtype == I8 else 448))     # some values clamp
    return x, scale


# (input shape, scale shape, wide form for 16-bit types?)
ELEMENTWISE_SHAPES = [((1, 128), (128,), True), ((7, 257), (257,), False), ((5, 1000), (1000,), True), ((32, 1024), (1024,), True),
                      ((3, 20000), (20000,), True), ((64, 8192), (8192,), True), ((2, 4, 128), (4, 128), True),
                      ((5, 2, 16, 32), (16, 32), True), ((3, 5, 12), (5, 12), False)]


@pytest.mark.parametrize("quant_dtype", [I8, F8], ids=str)
@pytest.mark.parametrize("dtype", U.NORM_DTYPES, ids=str)
@pytest.mark.parametrize("shapes", ELEMENTWISE_SHAPES, ids=str)
def test_static_quant_bit_exact(shapes, dtype, quant_dtype):
    shape, scale_shape, wide16 = shapes
    x, scale = static_inputs(shape, scale_shape, dtype, quant_dtype)
    numel = scale.numel()
    wide = numel % (16 // x.element_size()) == 0
    assert dtype == F32 or wide == wide16
    ref, op = static_pair(scale, quant_dtype)
    with torch.no_grad():
        want_q, _ = ref(x)
        xd = x.to(DEV)
        q, s = both_policies(lambda: op(xd), "static_quant:" + ("wide" if wide else "scalar"), has_nt=wide)
        assert q.dtype == quant_dtype and bit_equal(q, want_q) and torch.equal(s, scale)
        q, _ = to_cpu(op(misaligned(x)))                      # the same values behind a misaligned pointer: the scalar form
        assert last_launch() == "static_quant:scalar:cached" and bit_equal(q, want_q)
        if len(shape) == 2:                                   # a non-contiguous input
            wide_x = torch.cat([x, x], dim=-1).to(DEV)
            q, _ = to_cpu(op(wide_x[:, : shape[-1]]))
            assert bit_equal(q, want_q)


def dequant_inputs(shape, scale_shape, in_dtype):
    g = torch.Generator().manual_seed(sum(shape) + 1)
    if in_dtype == I8:
        q = torch.randint(-128, 128, shape, generator=g, dtype=torch.int32).to(I8)
    else:
        q = torch.randint(0, 256, shape, generator=g, dtype=torch.int32).to(torch.uint8).view(F8)     # every fp8 byte
        q = torch.where(q.float().isnan(), torch.zeros_like(q.float()), q.float()).to(F8)           # (but the two NaNs)
    return q, torch.rand(scale_shape, generator=g) * 0.05 + 1e-3


@pytest.mark.parametrize("in_dtype", [I8, F8], ids=str)
@pytest.mark.parametrize("out_dtype", U.NORM_DTYPES, ids=str)
@pytest.mark.parametrize("shapes", ELEMENTWISE_SHAPES, ids=str)
def test_dequant_bit_exact(shapes, out_dtype, in_dtype):
    shape, scale_shape, _ = shapes
    ref, op = U.golden_cls("MojoDequant")(output_dtype=out_dtype), hip_cls("MojoDequant")(output_dtype=out_dtype)
    for form, s_shape in (("trailing", scale_shape), ("token", shape[:-1] + (1,))):
        q, scale = dequant_inputs(shape, s_shape, in_dtype)
        period = scale.numel() if form == "trailing" else shape[-1]
        wide = period % 8 == 0
        want = ref(q, scale)
        qd, sd = on_dev(q, scale)
        got, = both_policies(lambda: op(qd, sd), f"dequant:{form}:{'wide' if wide else 'scalar'}", has_nt=wide)
        assert got.dtype == out_dtype and torch.equal(got, want), form
        got = to_cpu(op(misaligned(q), sd))
        assert last_launch() == f"dequant:{form}:scalar:cached", last_launch()
        assert torch.equal(got, want), f"{form}: {int((got != want).sum())} of {got.numel()} differ, first at {(got != want).flatten().nonzero()[:4].flatten().tolist()}"
        got = to_cpu(op(qd, sd.to(BF16)))                     # a 16-bit scale: .float() is exact
        assert torch.equal(got, ref(q, scale.to(BF16)))


def test_elementwise_grid_stride_second_trip():
    """More vectors than one trip of the capped grid (8192 workgroups x 256 threads): the scale index is carried by add-and-wrap
    from trip to trip.  bf16 in, so 8 elements per vector; the scale length is no divisor of the grid's stride."""
    trip = 8192 * 256
    dim = 4104                                                # rows of 513 vectors: the stride of a trip is no multiple of it
    rows = trip * 8 // dim + 4
    assert rows * dim // 8 > trip and trip % (dim // 8) != 0
    x, scale = static_inputs((rows, dim), (dim,), BF16, I8)
    ref, op = static_pair(scale, I8)
    with torch.no_grad():
        want_q, _ = ref(x)
        q, _ = to_cpu(op(x.to(DEV)))
    assert last_launch() == "static_quant:wide:cached" and torch.equal(q, want_q)
    deq, deq_ref = hip_cls("MojoDequant")(output_dtype=BF16), U.golden_cls("MojoDequant")(output_dtype=BF16)
    token_scale = torch.rand(rows, 1, generator=torch.Generator().manual_seed(5)) * 0.05 + 1e-3
    for s in (scale, token_scale):
        got = to_cpu(deq(want_q.to(DEV), s.to(DEV)))
        assert torch.equal(got, deq_ref(want_q, s))
    # the scalar forms: one element per thread, an odd row length
    x, scale = static_inputs((2100, 1001), (1001,), F16, I8)
    ref, op = static_pair(scale, I8)
    with torch.no_grad():
        want_q, _ = ref(x)
        q, _ = to_cpu(op(x.to(DEV)))
    assert last_launch() == "static_quant:scalar:cached" and torch.equal(q, want_q)
    token_scale = torch.rand(2100, 1, generator=torch.Generator().manual_seed(6)) * 0.05 + 1e-3
    for s, form in ((scale, "trailing"), (token_scale, "token")):
        got = to_cpu(deq(want_q.to(DEV), s.to(DEV)))
        assert last_launch() == f"dequant:{form}:scalar:cached" and torch.equal(got, deq_ref(want_q, s))


# ---- dequant -> SwiGLU -> quant -------------------------------------------------------------------------------------------------
def swiglu_pair(ws, qs, activate_left=False):
    kw = {"expert_num": ws.shape[0], "hidden_size": qs.shape[1], "activate_left": activate_left}
    state = {"weight_scale": ws, "quant_scale": qs}
    return (U.make_op(U.golden_cls("MojoDequantSwiGLUQuant"), state, **kw),
            U.make_op(hip_cls("MojoDequantSwiGLUQuant"), state, device=DEV, **kw))


def swiglu_tag(hidden, elt_bytes, aligned=True):
    wide = aligned and hidden % (16 // elt_bytes) == 0
    resident = hidden <= (14336 if wide else 4096)
    return f"dequant_swiglu_quant:{'wide' if wide else 'scalar'}:{'resident' if resident else 'reread'}"


@pytest.mark.parametrize("case", U.SWIGLU_SWEEP + [(5, 4099, None)], ids=str)
def test_dequant_swiglu_quant_reference_space(case):
    """int32 accumulators at every sweep shape: both `activate_left`, bias absent / shared / per expert, activation scale on and
    off, int32 and int64 counts; every launch form, cached and non-temporal; the scalar form behind a misaligned pointer gives
    the wide form's bits (the only reduction is a maximum)."""
    tokens, hidden, counts = case
    acc, act, ws, qs, bias, token_count = U.swiglu_inputs(tokens, hidden, None if counts is None else tuple(counts))
    tag = swiglu_tag(hidden, 4)
    differing = 0
    with torch.no_grad():
        for left in (False, True):
            ref, op = swiglu_pair(ws, qs, left)
            for b, a in ((None, act), (bias[0], None), (bias, act)):
                for count_dtype in (torch.int64, torch.int32):
                    tc = None if token_count is None else token_count.to(count_dtype)
                    want = ref(acc, a, b, None, tc)
                    args = on_dev(acc, a, b, None, tc)
                    got = both_policies(lambda: op(*args), tag, has_nt=":wide:" in tag)
                    differing += check_quant(*got, *want, I8, f"swiglu {case} left {left} bias {None if b is None else b.dim()}")
                    if ":wide:" in tag:
                        other = to_cpu(op(misaligned(acc), *args[1:]))
                        assert last_launch() == swiglu_tag(hidden, 4, aligned=False) + ":cached", last_launch()
                        assert torch.equal(other[0], got[0]) and torch.equal(other[1], got[1])
                    if token_count is None:
                        break
    print(f"swiglu {case}: {differing} differing quantised values in all")


@pytest.mark.parametrize("x_dtype", [torch.int32, F32, BF16, F16], ids=str)
def test_dequant_swiglu_quant_input_dtypes_and_device_side_grouping(x_dtype):
    """The four x dtypes; empty experts; counts that sum below T (tail rows: int8 zeros, scale 1); negative counts read as zero;
    the same integer values as int32 and as fp32 give the same bits."""
    tokens, hidden, counts = 40, 1000, (0, 25, 0, 15)
    acc, act, ws, qs, bias, _ = U.swiglu_inputs(tokens, hidden, counts)
    if x_dtype in (BF16, F16):
        acc = (acc // 64).clamp(-255, 255)                    # integers the 16-bit types hold exactly
        ws = ws * 64
    x = acc.to(x_dtype)
    assert torch.equal(x.float(), acc.float())
    tag = swiglu_tag(hidden, x.element_size())
    with torch.no_grad():
        ref, op = swiglu_pair(ws, qs)
        for tc in ([0, 25, 0, 15], [0, 20, 0, 11], [7, 0, 0, 0], [0, 0, 0, 0], [3, -4, 30, 50]):
            for count_dtype in (torch.int32, torch.int64):
                token_count = torch.tensor(tc, dtype=count_dtype)
                want = ref(x, act, bias, None, token_count)
                got = to_cpu(op(*on_dev(x, act, bias, None, token_count)))
                assert last_launch() == tag + ":cached", last_launch()
                check_quant(*got, *want, I8, f"swiglu {x_dtype} counts {tc}")
                live = min(sum(max(c, 0) for c in tc), tokens)
                assert not bool(got[0][live:].any()) and bool((got[1][live:] == 1.0).all())
                if x_dtype == F32:
                    as_int = to_cpu(op(*on_dev(acc, act, bias, None, token_count)))
                    assert torch.equal(as_int[0], got[0]) and torch.equal(as_int[1], got[1])
        # one expert, no token_count
        ref, op = swiglu_pair(ws[1:2], qs[1:2], True)
        check_quant(*to_cpu(op(*on_dev(x, act))), *ref(x, act), I8, f"swiglu {x_dtype} no counts")


def test_dequant_swiglu_quant_full_range_int32_rounds_as_int32_float():
    """|x| up to 2^30: the conversion is v_cvt_f32_i32, round to nearest even, as `int32.float()`; fed the rounded values as fp32
    the kernel gives the same bits."""
    tokens, hidden = 16, 512
    g = torch.Generator().manual_seed(30)
    x = torch.randint(-2 ** 30, 2 ** 30, (tokens, 2 * hidden), generator=g, dtype=torch.int64).to(torch.int32)
    x[0, :8] = torch.tensor([2 ** 24 + 1, 2 ** 24 + 3, -(2 ** 24 + 1), 2 ** 30 - 1, -(2 ** 30) + 1, 2 ** 25 + 2, 2 ** 25 + 6, 16777217])
    assert not torch.equal(x.float().to(torch.int64), x.to(torch.int64))        # the conversion does round
    ws = (torch.rand(1, 2 * hidden, generator=g) + 0.5) * 2.0 ** -28
    qs = torch.rand(1, hidden, generator=g) + 0.5
    act = torch.rand(tokens, generator=g) + 0.5
    with torch.no_grad():
        ref, op = swiglu_pair(ws, qs)
        want = ref(x, act)
        got = to_cpu(op(*on_dev(x, act)))
        check_quant(*got, *want, I8, "swiglu full-range int32")
        as_float = to_cpu(op(*on_dev(x.float(), act)))
    assert torch.equal(as_float[0], got[0]) and torch.equal(as_float[1], got[1])


# ---- rounding boundaries ------------------------------------------------------------------------------------------------------
def half_even(v, q_min, q_max):
    return torch.clamp(torch.round(v), q_min, q_max)


@pytest.mark.parametrize("dtype", [F16, F32], ids=str)
@pytest.mark.parametrize("quant_dtype", [I8, F8], ids=str)
def test_static_quant_rounding_boundaries(quant_dtype, dtype):
    """x / scale exactly k + 0.5 (scale a power of two per column): round half to even, which a reciprocal-multiply or a
    round-half-away would miss.  |k| <= 127 here: k + 0.5 is exact in fp16."""
    dim = 512
    scale = torch.tensor([2.0 ** -3, 2.0 ** -5, 0.25, 2.0])[torch.arange(dim) % 4]
    ties = (torch.arange(4 * dim) % 256 - 128).float().view(4, dim) + 0.5
    x = (ties * scale).to(dtype)
    assert torch.equal(x.float() / scale, ties)
    ref, op = static_pair(scale, quant_dtype)
    with torch.no_grad():
        want, _ = ref(x)
        q_max = 127 if quant_dtype == I8 else 448
        assert bit_equal(want, half_even(ties, -q_max - (quant_dtype == I8), q_max).to(quant_dtype))
        got, _ = to_cpu(op(x.to(DEV)))
    assert bit_equal(got, want)


@pytest.mark.parametrize("quant_dtype,symmetric", QUANT_KINDS, ids=str)
@pytest.mark.parametrize("name", ["MojoRMSNormQuant", "MojoLayerNormQuant", "MojoResidualAddLayerNormQuant"])
def test_norm_quant_rounding_boundaries(name, quant_dtype, symmetric):
    """`quant_dense_utils.norm_tie_case`: rows whose normalisation is exact, so that y / scale sits exactly on k + 0.5 with
    scale = 2^-4.  tests/test_quant_dense_golden.py checks the golden against the analytic round-half-even on these inputs; here
    the backend must give the golden's bits."""
    for dtype in (BF16, F32):
        state, kw, args, _ = U.norm_tie_case(name, quant_dtype, symmetric, dtype)
        ref, op = norm_pair(name, args[0].shape[-1], state, **kw)
        with torch.no_grad():
            want, got = ref(*args), to_cpu(op(*on_dev(*args)))
        assert bool((want[-1] == 2.0 ** -4).all())
        assert len(got) == len(want) and all(bit_equal(a, b) for a, b in zip(got, want)), (name, dtype)


@pytest.mark.parametrize("x_dtype", [torch.int32, F32], ids=str)
def test_dequant_swiglu_quant_rounding_boundaries(x_dtype):
    """gate = 64: expf(-64) vanishes beside 1, so silu(64) = 64 exactly on host and device; up = (2k + 1) * 2^-11, so
    z = (k + 0.5) * 2^-4 and one column carries 127 * 2^-4: z / scale = k + 0.5 exactly."""
    tokens, hidden = 5, 512
    k = (torch.arange(tokens * hidden) % 254 - 127).view(tokens, hidden)
    up = 2 * k + 1
    up[:, 3] = 254                                             # the row maximum: z = 127 * 2^-4
    x = torch.cat([up, torch.full((tokens, hidden), 64)], dim=1).to(x_dtype)        # [left = up | right = gate]
    ws = torch.cat([torch.full((1, hidden), 2.0 ** -11), torch.ones(1, hidden)], dim=1)
    qs = torch.ones(1, hidden)
    with torch.no_grad():
        ref, op = swiglu_pair(ws, qs)
        want = ref(x)
        assert bool((want[1] == 2.0 ** -4).all())
        expected = half_even(up.float() / 2, -128, 127).to(I8)
        assert torch.equal(want[0], expected), "the golden is off the analytic ties"
        got = to_cpu(op(x.to(DEV)))
    assert torch.equal(got[1], want[1]) and torch.equal(got[0], want[0])


# ---- the ops in sequence ------------------------------------------------------------------------------------------------------
def mlp_weights(hidden, inter, seed):
    g = torch.Generator().manual_seed(seed)
    w1 = torch.randn(hidden, 2 * inter, generator=g) * hidden ** -0.5          # [K, N]: gate | up
    w2 = torch.randn(inter, hidden, generator=g) * inter ** -0.5
    out = []
    for w in (w1, w2):
        scale = (w.abs().amax(0) / 127).to(BF16)
        out += [torch.clamp(torch.round(w / scale.float()), -128, 127).to(I8), scale]
    return w1, w2, out


def quant_gemm(cls, w_q, w_scale, device=None):
    op = cls(w_q.shape[0], w_q.shape[1], output_dtype=F32)
    with torch.no_grad():
        op.weight.copy_(w_q)
        op.weight_scale.copy_(w_scale)
    return op if device is None else op.to(device)


def test_graph_capture_of_norm_gemm_swiglu_equals_eager():
    """RMSNormQuant -> QuantGemm (fp32 out) -> DequantSwiGLUQuant captured in one graph and replayed on new activations: the
    eager bits, with nothing synchronising inside."""
    tokens, hidden, inter = 48, 512, 768
    _, _, (w1_q, w1_s, _, _) = mlp_weights(hidden, inter, 3)
    g = torch.Generator().manual_seed(4)
    norm = U.make_op(hip_cls("MojoRMSNormQuant"), {"weight": torch.rand(hidden, generator=g) + 0.5}, device=DEV, norm_size=hidden)
    gemm = quant_gemm(hip_cls("MojoQuantGemm"), w1_q, w1_s, DEV)
    stage = U.make_op(hip_cls("MojoDequantSwiGLUQuant"), {"weight_scale": torch.ones(1, 2 * inter), "quant_scale": torch.rand(1, inter, generator=g) + 0.5},
                      device=DEV, expert_num=1, hidden_size=inter)
    xs = [torch.randn(tokens, hidden, generator=g).to(BF16) for _ in range(3)]
    static_x = xs[0].to(DEV)

    def step():
        q, s = norm(static_x)
        return stage(gemm(q, s.reshape(-1)))

    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                          # warm-up outside the capture
            step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = step()
        for x in xs[1:]:
            static_x.copy_(x.to(DEV))
            graph.replay()
            torch.cuda.synchronize()
            replayed = [t.clone() for t in out]
            eager = step()
            torch.cuda.synchronize()
            assert torch.equal(replayed[0], eager[0]) and torch.equal(replayed[1], eager[1])
            assert bool(replayed[0].any())


def test_dense_w8a8_mlp_chain_stays_an_order_below_the_quantisation_error():
    """One dense W8A8 MLP at T 48, hidden 512, inter 768: RMSNormQuant, the gate|up int32 accumulators computed exactly on the
    host from the int8 bytes, DequantSwiGLUQuant (activation_scale = the norm's scale, weight_scale = the weight's), QuantGemm
    for the down projection.  max|hip - golden chain| <= 0.1 * max|golden chain - float MLP|."""
    tokens, hidden, inter = 48, 512, 768
    w1, w2, (w1_q, w1_s, w2_q, w2_s) = mlp_weights(hidden, inter, 7)
    g = torch.Generator().manual_seed(8)
    x = torch.randn(tokens, hidden, generator=g).to(BF16)
    norm_w = torch.rand(hidden, generator=g) + 0.5

    def chain(cls_of, device):
        norm = U.make_op(cls_of("MojoRMSNormQuant"), {"weight": norm_w}, device=device, norm_size=hidden)
        # SwiGLU of the MLP: silu(gate) * up with gate FIRST -> activate_left
        stage = U.make_op(cls_of("MojoDequantSwiGLUQuant"), {"weight_scale": w1_s.float().view(1, -1), "quant_scale": torch.ones(1, inter)},
                          device=device, expert_num=1, hidden_size=inter, activate_left=True)
        down = quant_gemm(cls_of("MojoQuantGemm"), w2_q, w2_s, device)
        q, s = norm(x.to(device))
        acc = (q.cpu().to(torch.int64) @ w1_q.to(torch.int64)).to(torch.int32).to(device)      # exact: |acc| < 2^31
        h_q, h_s = stage(acc, s.reshape(-1))
        return down(h_q, h_s.reshape(-1)).cpu()

    with torch.no_grad():
        got = chain(hip_cls, DEV)
        want = chain(torch_cls, "cpu")
        normed = torch.nn.functional.rms_norm(x.float(), [hidden], weight=norm_w, eps=1e-5)
        gate_up = normed @ w1
        exact = (torch.nn.functional.silu(gate_up[:, :inter]) * gate_up[:, inter:]) @ w2
    backend_error = float((got - want).abs().max())
    quantisation_error = float((want - exact).abs().max())
    print(f"dense W8A8 MLP: max|hip - golden chain| {backend_error:.3e}, max|golden chain - float MLP| {quantisation_error:.3e}, "
          f"ratio {backend_error / quantisation_error:.3e}")
    assert quantisation_error > 0 and backend_error <= 0.1 * quantisation_error
