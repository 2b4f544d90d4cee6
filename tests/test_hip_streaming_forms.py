"""Every launch form of the streaming kernels (rmsnorm.hip, norm_quant.hip, swiglu.hip): each case asserts the
`mojo_hip_last_launch()` tag it is about, compares with the CPU golden, and runs once more with MOJO_HIP_STREAM_NT=1 — the
non-temporal twin says `nt` and gives the bits of the cached run (the policy changes loads and stores, not arithmetic).

Shapes are for the 16-bit types; fp32 halves `dim` of the 16-byte-vector ("wide") forms, which keeps the number of vectors
per row, and keeps the shape of the others.  `@k`: a contiguous view that starts at element k of a flat buffer.

  tag                                   case
  rmsnorm:vec8|vec4:tpr64               rms  5x64 (rows no multiple of 4), 32771x8 (second grid-stride trip, dead row group)
  rmsnorm:vec8|vec4:tpr128              rms  131x2056 (a dead half-workgroup beside a live one; in place too)
  rmsnorm:vec8|vec4:tpr256              rms  3x2048, 130x4104, 9x8200 (past the register cache; in place too)
  rmsnorm:vec2:tpr64 / tpr128 / tpr256  rms  5x64@2 / 5x738 / 5x1032@2
  rmsnorm:vec1:tpr64 / tpr128 / tpr256  rms  5x64@1 / 5x264@1 / 33x1031 (re-read), 8195x513 (second trip)
  norm_quant:wide:tpr64                 dynamic quant 2051x8, 2049x2048 (four live vectors per lane), 32773x8 (second trip)
  norm_quant:wide:tpr256                dynamic quant 7x1024, 64x1024 (fp32: four-byte packing), 3x8200 (past the cache);
                                        norm+quant 52x1024, 7x8200, 8195x8 (second trip)
  norm_quant:scalar:tpr256              dynamic quant 64x1001, 32x2051 (past its cache of 8), 8195x7 (second trip), 16x1024@1;
                                        norm+quant 52x1001
  swiglu:wide                           n = 8 * (1024 + 5) (full trip + plain-stored partial trip), n = 8 * 1024
  swiglu:scalar                         9x999, n = 4096 * 1024 + 7 (second trip)
  swiglu_rows:wide / scalar             the halves of a fused 37 x 528 projection: 264 columns / 101 columns
  (`:nt` / `:cached` ends every tag but swiglu_rows'; the scalar forms have no non-temporal twin and always say `cached`)

The rounding-boundary rows of the dynamic quantiser come from a scan on the CPU (`boundary_scan`): row maxima at the bf16 bit
patterns 0x3F80 ... 0x41FF in steps of 3, y over every positive bf16 <= the maximum; the hits are the y where the fp32
shortcut rint(y * (1 / scale)) differs from rint(y / scale) and the y whose exact quotient is k + 0.5.
"""
import functools

import pytest
import torch

from hip_utils import DEV, hip_cls, last_launch, max_ulp_bf16ish, switch_env, to_cpu, torch_cls

pytestmark = pytest.mark.gpu

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = [pytest.param(BF16, id="bf16"), pytest.param(F16, id="fp16"), pytest.param(F32, id="fp32")]


def misaligned(t, offset, device=DEV):
    """``t``'s values in a contiguous view that starts ``offset`` elements into a fresh flat buffer on ``device``."""
    if not offset:
        return t.to(device)
    flat = torch.empty(t.numel() + offset, dtype=t.dtype, device=device)
    view = flat[offset:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == (offset * t.element_size()) % 16
    return view


def both_policies(run, tag, has_nt=True):
    """``run()`` with MOJO_HIP_STREAM_NT=0, then =1: the tags (``tag`` + ':cached' / ':nt'; ``has_nt`` False: a form without
    a non-temporal twin, the same tag twice), and the second run's outputs equal to the first's bit for bit.  Returns the
    cached run's outputs on the CPU."""
    with switch_env(MOJO_HIP_STREAM_NT="0"):
        cached = run()
        assert last_launch() == tag + ":cached", (last_launch(), tag)
    with switch_env(MOJO_HIP_STREAM_NT="1"):
        streamed = run()
        assert last_launch() == tag + (":nt" if has_nt else ":cached"), (last_launch(), tag)
    cached, streamed = to_cpu(cached), to_cpu(streamed)
    assert len(cached) == len(streamed) and all(torch.equal(a, b) for a, b in zip(cached, streamed)), tag
    return cached


# ---- RMSNorm family ------------------------------------------------------------------------------------------------
# (id, rows, dim for 16-bit types, wide form?, element offset of hidden / residual, vector elements (0: the wide width), threads
#  per row, in place too?)
RMS_FORMS = [
    ("wave", 5, 64, True, 0, 0, 64, False),
    ("two-waves", 131, 2056, True, 0, 0, 128, True),
    ("block-few-rows", 3, 2048, True, 0, 0, 256, False),
    ("block", 130, 4104, True, 0, 0, 256, False),
    ("block-reread", 9, 8200, True, 0, 0, 256, True),
    ("scalar-reread", 33, 1031, False, 0, 1, 256, False),
    ("pairs", 5, 738, False, 0, 2, 128, False),
    ("at1-wave", 5, 64, False, 1, 1, 64, False),
    ("at1-two-waves", 5, 264, False, 1, 1, 128, False),
    ("at2-wave", 5, 64, False, 2, 2, 64, False),
    ("at2-block", 5, 1032, False, 2, 2, 256, False),
    ("wave-second-trip", 32771, 8, True, 0, 0, 64, False),
    ("scalar-second-trip", 8195, 513, False, 0, 1, 256, False),
]
RMS_CAP = {"wave-second-trip": 8192 * 4, "scalar-second-trip": 8192}       # rows of one trip of the capped grid


def rms_inputs(form, dtype):
    name, rows, dim, wide, offset, vec, tpr, inplace = form
    if wide and dtype == F32:
        dim //= 2
    g = torch.Generator().manual_seed(rows * 7 + dim)
    x, r = torch.randn(rows, dim, generator=g).to(dtype), torch.randn(rows, dim, generator=g).to(dtype)
    w = torch.randn(dim, generator=g).to(dtype)
    return x, r, w


def rms_goldens(x, r, w, dtype, eps=1e-5):
    """{kind: golden outputs}: the residual-add norm (`pre` returns (normed, summed); `post` the same normed twice) and the
    plain norm of x (MojoRMSNorm; MojoRMSNormInplace returns the same values)."""
    dim = x.shape[-1]
    ref = torch_cls("MojoResidualAddRMSNorm")(dim, eps, "pre", dtype=dtype)
    plain = torch_cls("MojoRMSNorm")(dim, eps, dtype=dtype)
    with torch.no_grad():
        ref.weight.copy_(w)
        plain.weight.copy_(w)
        normed, summed = ref(x, r)
        return {"pre": (normed, summed), "post": (normed,), "norm": (plain(x),), "inplace": (plain(x),)}


def normed_error(got, want):
    """Worst error of a normed tensor in units of the last place for the 16-bit types (the bound is 1: fp32 math, one
    rounding); fp32 is asserted within the project's 2e-5 and its worst error relative to max(|want|, 1) returned."""
    if want.dtype == F32:
        torch.testing.assert_close(got, want, atol=2e-5, rtol=2e-5)
        return float(((got - want).abs() / want.abs().clamp_min(1.0)).max())
    return max_ulp_bf16ish(got, want)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", [pytest.param(f, id=f[0]) for f in RMS_FORMS])
def test_rmsnorm_forms(form, dtype):
    name, rows, dim, wide, offset, vec, tpr, inplace = form
    x, r, w = rms_inputs(form, dtype)
    dim = x.shape[-1]
    tag = f"rmsnorm:vec{vec or 16 // x.element_size()}:tpr{tpr}"
    want = rms_goldens(x, r, w, dtype)
    ops = {"pre": hip_cls("MojoResidualAddRMSNorm")(dim, 1e-5, "pre", dtype=dtype, device=DEV),
           "post": hip_cls("MojoResidualAddRMSNorm")(dim, 1e-5, "post", dtype=dtype, device=DEV),
           "norm": hip_cls("MojoRMSNorm")(dim, 1e-5, dtype=dtype, device=DEV)}
    if inplace:
        ops["inplace"] = hip_cls("MojoRMSNormInplace")(dim, 1e-5, inplace=True, dtype=dtype, device=DEV)
    with torch.no_grad():
        for op in ops.values():
            op.weight.copy_(w)

    def call(kind):
        xd = misaligned(x, offset)                              # (a fresh copy: the in-place op overwrites it)
        if kind in ("pre", "post"):
            out = ops[kind](xd, misaligned(r, offset))
            return out if kind == "pre" else out[:1]
        out = ops[kind](xd)
        assert (out.data_ptr() == xd.data_ptr()) == (kind == "inplace")
        return (out,)

    worst = 0.0
    for kind in ops:
        got = both_policies(lambda: call(kind), tag)
        if offset:                                              # the same values behind aligned pointers: the wide form
            with switch_env(MOJO_HIP_STREAM_NT="0"):
                aligned = to_cpu(ops[kind](x.to(DEV), r.to(DEV)) if kind in ("pre", "post") else (ops[kind](x.to(DEV)),))
                assert last_launch().startswith(f"rmsnorm:vec{16 // x.element_size()}:"), last_launch()
            print(f"rmsnorm {name} {kind} {dtype}: {int((aligned[0] != got[0]).sum())} of {got[0].numel()} differ from the aligned call")
            assert kind != "pre" or torch.equal(aligned[1], got[1])
            if dtype == F32:
                # the vector width decides which elements a lane squares and adds first: another fp32 summation order, so
                # the row statistic moves in its last place and every fp32 output of the row with it (measured: 58 to 880
                # elements of these cases differ, all in the last place); the 16-bit outputs round that away
                torch.testing.assert_close(got[0], aligned[0], atol=2e-5, rtol=2e-5)
            else:
                assert torch.equal(aligned[0], got[0])
        worst = max(worst, normed_error(got[0], want[kind][0]))
        if kind == "pre":
            assert torch.equal(got[1], want[kind][1])           # the sum: a plain rounded add
        if name in RMS_CAP:                                     # first, last and cap-adjacent rows, one by one
            for row in (0, RMS_CAP[name] - 1, RMS_CAP[name], rows - 1):
                assert dtype == F32 or normed_error(got[0][row], want[kind][0][row]) <= 1, (kind, row)
                assert kind != "pre" or torch.equal(got[1][row], want[kind][1][row]), (kind, row)
    print(f"rmsnorm {name} {tuple(x.shape)} {dtype}: worst {'rel err' if dtype == F32 else 'ulp'} {worst:.3g}")
    assert dtype == F32 or worst <= 1, worst


# ---- dynamic quant ---------------------------------------------------------------------------------------------------
# (id, rows, dim for 16-bit types, dim for fp32, element offset of the input, tag)
DQ_FORMS = [
    ("wave", 2051, 8, 4, 0, "norm_quant:wide:tpr64"),
    ("wave-full-cache", 2049, 2048, 1024, 0, "norm_quant:wide:tpr64"),
    ("wave-second-trip", 32773, 8, 4, 0, "norm_quant:wide:tpr64"),
    ("block", 7, 1024, 512, 0, "norm_quant:wide:tpr256"),
    ("block-1024", 64, 1024, 1024, 0, "norm_quant:wide:tpr256"),
    ("block-reread", 3, 8200, 4100, 0, "norm_quant:wide:tpr256"),
    ("scalar", 64, 1001, 1001, 0, "norm_quant:scalar:tpr256"),
    ("scalar-reread", 32, 2051, 2051, 0, "norm_quant:scalar:tpr256"),
    ("scalar-second-trip", 8195, 7, 7, 0, "norm_quant:scalar:tpr256"),
    ("at1", 16, 1024, 1024, 1, "norm_quant:scalar:tpr256"),
]
DQ_PARAMS = [pytest.param(f, id=f[0]) for f in DQ_FORMS]


def dq_pair(dim, inv_smooth):
    """(golden, HIP op) of MojoDynamicQuant, with ``inv_smooth`` [dim] fp32 or None."""
    ref = torch_cls("MojoDynamicQuant")(input_size=None if inv_smooth is None else dim)
    op = hip_cls("MojoDynamicQuant")(input_size=None if inv_smooth is None else dim)
    if inv_smooth is not None:
        with torch.no_grad():
            ref.inv_smooth_scale.copy_(inv_smooth)
        op = op.to(DEV)
        op.load_state_dict(ref.state_dict())
    return ref, op


def check_dynamic_quant(x, inv_smooth, offset, tag):
    """Both policies of the form ``tag``, bit-exact against the golden; returns the golden's (q, scale)."""
    ref, op = dq_pair(x.shape[-1], inv_smooth)
    with torch.no_grad():
        want_q, want_scale = ref(x)
    xd = misaligned(x, offset)
    q, scale = both_policies(lambda: op(xd), tag, has_nt=":wide:" in tag)
    assert q.dtype == torch.int8 and scale.dtype == F32 and scale.shape == want_scale.shape
    assert torch.equal(scale, want_scale)
    assert torch.equal(q, want_q), f"{int((q != want_q).sum())} of {q.numel()} bytes differ from the golden"
    return want_q, want_scale


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", DQ_PARAMS)
def test_dynamic_quant_forms_bit_exact(form, dtype):
    name, rows, dim16, dim32, offset, tag = form
    dim = dim32 if dtype == F32 else dim16
    g = torch.Generator().manual_seed(rows + dim)
    x = torch.randn(rows, dim, generator=g).to(dtype)
    check_dynamic_quant(x, None, offset, tag)
    check_dynamic_quant(x, 1.0 / (torch.rand(dim, generator=g) + 0.1), offset, tag)


# ---- rounding boundaries of the dynamic quantiser ------------------------------------------------------------------------
def shortcut_differs(y, amax):
    """Where fp32 rint(y * (1 / scale)) != rint(y / scale), scale = amax / 127 (the golden's operations, IEEE single)."""
    scale = amax.clamp(min=1e-12) / 127
    return torch.round(y * (1.0 / scale)) != torch.round(y / scale)


def exact_tie(y, amax):
    """Where the real quotient 127 y / amax is k + 0.5: 254 y / amax an odd integer (254 y and odd * amax are exact in fp64
    for values of at most 24 significant bits, so the product check decides it)."""
    y, amax = y.double().abs(), amax.double()
    twice = (y * 254) / amax
    return (twice == twice.floor()) & (twice % 2 == 1) & (twice * amax == y * 254)


@functools.lru_cache(None)
def boundary_scan():
    """[(amax, hits)]: for every scanned row maximum with a hit, the positive bf16 y <= amax (as fp32) where the shortcut
    alone gives the wrong integer or the exact quotient is a tie; plus the two counts."""
    out, n_differs, n_ties = [], 0, 0
    for bits in range(0x3F80, 0x4200, 3):
        amax = torch.tensor([bits], dtype=torch.int16).view(BF16).float()
        y = torch.arange(1, bits + 1, dtype=torch.int16).view(BF16).float()
        differs, ties = shortcut_differs(y, amax), exact_tie(y, amax)
        n_differs, n_ties = n_differs + int(differs.sum()), n_ties + int(ties.sum())
        if bool((differs | ties).any()):
            out.append((float(amax), y[differs | ties]))
    return out, n_differs, n_ties


def tiny_rows(dim, dtype, g):
    """Four rows around the `scale < 1e-6 -> 1.0` branch: zeros, 1e-5 everywhere, and two whose amax / 127 is the last value of
    ``dtype`` below and the first at or above 1e-6 (the other elements: fractions of that maximum)."""
    ints = torch.int32 if dtype == F32 else torch.int16
    v = torch.tensor([1.27e-4]).to(dtype)
    scale_of = lambda t: t.float().clamp(min=1e-12) / 127                                       # noqa: E731
    while bool(scale_of(v) >= 1e-6):
        v = (v.view(ints) - 1).view(dtype)
    while bool(scale_of((v.view(ints) + 1).view(dtype)) < 1e-6):
        v = (v.view(ints) + 1).view(dtype)
    below, above = v, (v.view(ints) + 1).view(dtype)
    assert bool(scale_of(below) < 1e-6) and bool(scale_of(above) >= 1e-6)
    rows = torch.zeros(4, dim)
    rows[1] = 1e-5
    for i, top in ((2, below), (3, above)):
        rows[i] = (torch.rand(dim, generator=g) * 2 - 1) * float(top)
        rows[i, int(torch.randint(dim, (1,), generator=g))] = float(top)
    return rows.to(dtype)


def assert_tiny_rows_straddle(scale):
    """The golden's scales of `tiny_rows`: 1.0 three times, then the first fp32 scale that is not below 1e-6."""
    last4 = scale[-4:].flatten()
    assert last4[:3].tolist() == [1.0, 1.0, 1.0] and bool(last4[3] >= torch.tensor(1e-6)) and float(last4[3]) < 1.01e-6, last4


def boundary_row_count(dim):
    """Rows that `boundary_rows` needs to hold every hit once."""
    return sum(-(-2 * len(ys) // (dim - 1)) for _, ys in boundary_scan()[0]) + 4


def boundary_rows(rows, dim, dtype, seed):
    """[rows, dim] of ``dtype``, fp32 values y: every row holds one maximum of the scan, that maximum's hits with both
    signs (as many as fit; the rest go to further rows) at random columns — near-boundary elements share their vectors
    with far ones — and random padding below the maximum; the rows repeat to fill ``rows``; the last four are `tiny_rows`."""
    scan, _, _ = boundary_scan()
    g = torch.Generator().manual_seed(seed)
    units = [(amax, chunk) for amax, ys in scan for chunk in torch.cat([ys, -ys]).split(dim - 1)]
    assert rows >= len(units) + 4 == boundary_row_count(dim), (rows, len(units))
    base = torch.empty(len(units), dim)
    for i, (amax, chunk) in enumerate(units):
        row = ((torch.rand(dim, generator=g) * 2 - 1) * amax).to(BF16).float()
        at = torch.randperm(dim, generator=g)
        row[at[0]] = amax if i % 2 else -amax
        row[at[1: 1 + len(chunk)]] = chunk
        base[i] = row
    y = base.repeat((rows - 4 + len(units) - 1) // len(units), 1)[: rows - 4].to(dtype)    # (the hits are exact in fp16 too)
    return torch.cat([y, tiny_rows(dim, dtype, g)])


def assert_boundary_input(y):
    """The precondition of the boundary tests, on the fp32 values the quantiser divides: at least 30 distinct (maximum, |y|)
    pairs where the shortcut alone is wrong and at least 200 exact ties (the bf16 scan yields 37 and 466)."""
    amax = y.abs().amax(dim=-1, keepdim=True)
    counted = (amax.clamp(min=1e-12) / 127 >= 1e-6).expand_as(y)          # (rows below that take scale = 1.0)
    pairs = lambda mask: len(torch.unique(torch.stack([amax.expand_as(y)[mask], y[mask].abs()], dim=1), dim=0))   # noqa: E731
    n_differs, n_ties = pairs(shortcut_differs(y, amax) & counted), pairs(exact_tie(y, amax) & counted)
    assert n_differs >= 30 and n_ties >= 200, (n_differs, n_ties)
    return n_differs, n_ties


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", DQ_PARAMS)
def test_dynamic_quant_rounding_boundaries_bit_exact(form, dtype):
    """Inputs whose quotients sit ON the rounding boundaries (exact ties, and values where the reciprocal shortcut alone
    rounds to the other side), in every launch form, with and without a power-of-two smooth scale (the quotients are the
    same); the last four rows take the `scale < 1e-6 -> 1.0` branch or just miss it."""
    name, rows, dim16, dim32, offset, tag = form
    dim = dim32 if dtype == F32 else dim16
    need = boundary_row_count(dim)
    rows = max(rows, need) if rows >= 2048 else need        # (the forms of fewer than 2048 rows: no more than they need)
    assert ":tpr64" in tag or rows < 2048 or ":scalar:" in tag
    y = boundary_rows(rows, dim, dtype, seed=rows + dim)
    assert_boundary_input(y.float())
    _, want_scale = check_dynamic_quant(y, None, offset, tag)
    assert_tiny_rows_straddle(want_scale)
    g = torch.Generator().manual_seed(dim)
    inv = torch.tensor([1.0, 0.5, 0.25])[torch.randint(3, (dim,), generator=g)]
    x = (y.float() / inv).to(dtype)
    assert torch.equal(x.float() * inv, y.float())                          # exact: the same quotients
    _, want_scale = check_dynamic_quant(x, inv, offset, tag)
    assert_tiny_rows_straddle(want_scale)


def moe_boundary_rows(dim, dtype, experts=3):
    """(y, inv, counts) of the MoE boundary tests: `boundary_rows` of ``dim`` columns as the smoothed values, power-of-two
    smooth scales per expert and column (so y / inv and back is exact), the rows split over the first and the last expert."""
    y = boundary_rows(boundary_row_count(dim), dim, dtype, seed=dim)
    assert_boundary_input(y.float())
    g = torch.Generator().manual_seed(dim)
    inv = torch.tensor([1.0, 0.5, 0.25])[torch.randint(3, (experts, dim), generator=g)]
    counts = torch.tensor([y.shape[0] // 2, 0, y.shape[0] - y.shape[0] // 2], dtype=torch.int32)
    return y, inv, counts


def check_moe_plain_boundaries(dim, form, dtype):
    """MojoMoEDynamicQuant on `moe_boundary_rows`: the launch tag, and scale and bytes equal to the golden's."""
    y, inv, counts = moe_boundary_rows(dim, dtype)
    smooth_rows = inv.repeat_interleave(counts, dim=0)
    x = (y.float() / smooth_rows).to(dtype)
    assert torch.equal(x.float() * smooth_rows, y.float())
    ref = torch_cls("MojoMoEDynamicQuant")(len(counts), dim)
    with torch.no_grad():
        ref.inv_smooth_scale.copy_(inv)
        want_q, want_scale = ref(x, counts)
    op = hip_cls("MojoMoEDynamicQuant")(len(counts), dim).to(DEV)
    op.load_state_dict(ref.state_dict())
    q, scale = to_cpu(op(x.to(DEV), counts.to(DEV)))
    assert last_launch() == "moe_quant:plain:" + form, last_launch()
    assert torch.equal(scale, want_scale) and torch.equal(q, want_q)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim,form", [(1024, "vec16"), (1001, "scalar")])
def test_moe_dynamic_quant_rounding_boundaries_bit_exact(dim, form, dtype):
    """MojoMoEDynamicQuant takes the reciprocal shortcut; the boundary rows hold it to its exact-division fallback."""
    check_moe_plain_boundaries(dim, form, dtype)


# (dim for bf16 and fp16, dim for fp32, form): 1025 vectors, one past the 4 x 256 a workgroup keeps; 7 columns past the 1024
MOE_REREAD = [(8200, 4100, "vec16"), (1031, 1031, "scalar")]
# the glu form on the resident rows too
MOE_GLU = MOE_REREAD + [(1024, 1024, "vec16"), (1001, 1001, "scalar")]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim16,dim32,form", MOE_REREAD)
def test_moe_dynamic_quant_reread_tail_rounding_boundaries_bit_exact(dim16, dim32, form, dtype):
    """The boundary rows in rows longer than the register cache: the vectors past it are recomputed and quantised by the
    tail loop, whose shortcut needs its fallback like the cached part's."""
    check_moe_plain_boundaries(dim32 if dtype == F32 else dim16, form, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim16,dim32,form", MOE_GLU)
def test_moe_swiglu_quant_rounding_boundaries_bit_exact(dim16, dim32, form, dtype):
    """The glu form on the same quotients: gate = 32, where silu is the identity in fp32 (expf(-32) is below half an ulp of
    1, so 32 / (1 + expf(-32)) = 32), up = y / inv and the op's smooth scale inv / 32, all powers of two apart: silu(gate) *
    up * (inv / 32) = y with no rounding anywhere, which the test asserts before it compares."""
    from mojo_opset_amd.backends.hip.operators.quantize import moe_dynamic_quant
    dim = dim32 if dtype == F32 else dim16
    y, inv, counts = moe_boundary_rows(dim, dtype)
    smooth = inv / 32
    smooth_rows = smooth.repeat_interleave(counts, dim=0)
    gate = torch.full(y.shape, 32.0).to(dtype)
    up = (y.float() / inv.repeat_interleave(counts, dim=0)).to(dtype)
    activated = torch.nn.functional.silu(gate.float()) * up.float()
    assert torch.equal(activated * smooth_rows, y.float())
    ref = torch_cls("MojoMoEDynamicQuant")(len(counts), dim)
    with torch.no_grad():
        ref.inv_smooth_scale.copy_(smooth)
        want_q, want_scale = ref(activated, counts)
    x = torch.cat([gate, up], dim=-1).contiguous()
    q, scale = to_cpu(moe_dynamic_quant(x.to(DEV), smooth.to(DEV), counts.to(DEV), dim, True, "test"))
    assert last_launch() == "moe_quant:swiglu:" + form, last_launch()
    assert_tiny_rows_straddle(want_scale)
    assert torch.equal(scale, want_scale) and torch.equal(q, want_q)


# ---- norm + quant ----------------------------------------------------------------------------------------------------
# (id, rows, dim, tag): at least 50 000 elements each — the 2e-3 share of differing bytes needs them to mean anything
NQ_FORMS = [
    ("block", 52, 1024, "norm_quant:wide:tpr256"),
    ("scalar", 52, 1001, "norm_quant:scalar:tpr256"),
    ("block-reread", 7, 8200, "norm_quant:wide:tpr256"),
    ("block-second-trip", 8195, 8, "norm_quant:wide:tpr256"),
]
NQ_COMBOS = [(pos, qd, smooth) for pos in ("pre", "post") for qd in (torch.int8, torch.float8_e4m3fn) for smooth in (False, True)]


def nq_inputs(form, dtype):
    name, rows, dim, tag = form
    assert rows * dim >= 50000
    g = torch.Generator().manual_seed(rows + dim)
    x, r = torch.randn(rows, dim, generator=g).to(dtype), torch.randn(rows, dim, generator=g).to(dtype)
    return x, r, torch.randn(dim, generator=g), torch.rand(dim, generator=g) + 0.5


def nq_golden(x, r, w, smooth, pos, qd):
    ref = torch_cls("MojoResidualAddRMSNormQuant")(norm_size=x.shape[-1], norm_pos=pos, quant_dtype=qd)
    with torch.no_grad():
        ref.weight.copy_(w)
        return ref, ref(x, r, smooth)


def nq_differing(q, want_q, qd):
    """(largest difference of the quantised values, share of elements that differ)."""
    diff = (q.float() - want_q.float()).abs()
    return float(diff.max()), float((diff > 0).float().mean())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", [pytest.param(f, id=f[0]) for f in NQ_FORMS])
def test_rmsnorm_quant_forms(form, dtype):
    from test_hip_quantizers import _check_norm_quant
    name, rows, dim, tag = form
    x, r, w, smooth_scale = nq_inputs(form, dtype)
    worst = 0.0
    for pos, qd, with_smooth in NQ_COMBOS:
        smooth = smooth_scale if with_smooth else None
        ref, want = nq_golden(x, r, w, smooth, pos, qd)
        op = hip_cls("MojoResidualAddRMSNormQuant")(norm_size=dim, norm_pos=pos, quant_dtype=qd).to(DEV)
        op.load_state_dict(ref.state_dict())
        xd, rd, sd = x.to(DEV), r.to(DEV), None if smooth is None else smooth.to(DEV)
        got = both_policies(lambda: op(xd, rd, sd), tag, has_nt=":wide:" in tag)
        _check_norm_quant(got, want, qd)
        worst = max(worst, nq_differing(got[0], want[0], qd)[1])
    print(f"norm+quant {name} {tuple(x.shape)} {dtype}: largest share of differing elements {worst:.2e}")


# ---- SwiGLU ----------------------------------------------------------------------------------------------------------
def swiglu_check(make, tag, dtype, limit, has_nt):
    """``make(device)`` -> (gate, up) views on that device, of the same values."""
    gate, up = make("cpu")
    with torch.no_grad():
        want = torch_cls("MojoSwiGLU")(swiglu_limit=limit)(gate, up)
    op = hip_cls("MojoSwiGLU")(swiglu_limit=limit)
    gd, ud = make(DEV)
    with switch_env(MOJO_HIP_STREAM_NT="0"):
        got = op(gd, ud)
        assert last_launch() == tag + (":cached" if has_nt is not None else ""), last_launch()
    with switch_env(MOJO_HIP_STREAM_NT="1"):
        streamed = op(gd, ud)
        assert last_launch() == tag + {True: ":nt", False: ":cached", None: ""}[has_nt], last_launch()
    assert torch.equal(got, streamed)
    got = to_cpu(got)
    assert got.shape == want.shape and got.dtype == want.dtype
    if dtype == F32:
        torch.testing.assert_close(got, want, atol=1e-5, rtol=1e-5)
        return
    worst = max_ulp_bf16ish(got, want)
    print(f"swiglu {tag} {tuple(want.shape)} {dtype} limit {limit}: worst ulp {worst:.3g}")
    assert worst <= 1, worst


def off_the_silu_ties(gate, limit):
    """``gate`` with the values moved one step up whose silu the 16-bit golden cannot round reliably.  The golden rounds
    silu(gate) to the storage type BEFORE the multiply.  Where the exact silu lies within the error of an fp32 evaluation of a
    rounding tie of that type, the side is decided by the last bits of whichever exp is used — the host's libm in the golden,
    v_exp_f32 / v_rcp_f32 in the kernel — and the product then differs by up to two last places although both evaluated silu
    to fp32 accuracy (bf16 5.9375: silu = 5.92187444, the tie between 5.90625 and 5.9375 is 5.921875).  The window is the
    kernel's fp32 error bound: half an ulp of gate * log2(e), which the exponential turns into |gate| ulps, one ulp each
    for exp2 and the reciprocal, half an ulp each for the add and the multiply — (|gate| + 4) * 2^-24 relative, doubled
    for the golden's own error.  fp32 has no such rounding."""
    if gate.dtype == F32:
        return gate
    mant, e_min = {BF16: (7, -126), F16: (10, -14)}[gate.dtype]
    for _ in range(8):
        g = gate.double()
        if limit > 0:
            g = g.clamp(max=limit)
        s = g / (1 + torch.exp(-g))
        step = torch.pow(2.0, torch.floor(torch.log2(s.abs().clamp_min(2.0 ** -140))).clamp_min(e_min) - mant)
        from_tie = ((s.abs() / step) % 1 - 0.5).abs() * step
        unsure = from_tie < 2 * (g.abs() + 4) * 2.0 ** -24 * s.abs()
        if not bool(unsure.any()):
            return gate
        bits = gate.view(torch.int16)
        gate = torch.where(unsure, bits + torch.where(gate >= 0, 1, -1).to(torch.int16), bits).view(gate.dtype)
    raise AssertionError("gates still on a silu rounding tie")


def _flat_pair(n, dtype, seed, limit):
    g = torch.Generator().manual_seed(seed)
    gate, up = (torch.randn(n, generator=g) * 2).to(dtype), (torch.randn(n, generator=g) * 2).to(dtype)
    gate = off_the_silu_ties(gate, limit)
    return lambda device: (gate.to(device), up.to(device))


# (id, number of 16-byte vectors (wide forms) or of elements, wide?)
SWIGLU_DENSE = [("full-and-partial-trip", 1024 + 5, True), ("one-full-trip", 1024, True), ("scalar-9x999", 9 * 999, False),
                ("scalar-second-trip", 4096 * 1024 + 7, False)]


@pytest.mark.parametrize("limit", [0.0, 1.5])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [pytest.param(c, id=c[0]) for c in SWIGLU_DENSE])
def test_swiglu_dense_forms(case, dtype, limit):
    name, count, wide = case
    n = count * (16 // torch.empty(0, dtype=dtype).element_size()) if wide else count
    make = _flat_pair(n, dtype, count, limit)
    if name == "scalar-9x999":
        flat = make
        make = lambda device: tuple(t.view(9, 999) for t in flat(device))                     # noqa: E731
    swiglu_check(make, "swiglu:wide" if wide else "swiglu:scalar", dtype, limit, has_nt=wide)


@pytest.mark.parametrize("limit", [0.0, 1.5])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cols,tag", [(264, "swiglu_rows:wide"), (101, "swiglu_rows:scalar")])
def test_swiglu_row_strided_forms(cols, tag, dtype, limit):
    """The two halves of a fused [37, 2 * 264] projection, read where they are: whole halves (16-byte vectors) and their
    first 101 columns (an odd count: element by element)."""
    g = torch.Generator().manual_seed(cols)
    gu = (torch.randn(37, 2 * 264, generator=g) * 2).to(dtype)
    gu[:, :264] = off_the_silu_ties(gu[:, :264].contiguous(), limit)

    def make(device):
        t = gu.to(device)
        gate, up = t[:, :cols], t[:, 264: 264 + cols]
        assert not gate.is_contiguous() and not up.is_contiguous()
        return gate, up

    swiglu_check(make, tag, dtype, limit, has_nt=None)
