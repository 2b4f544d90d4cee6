"""The DiT block ops on the GPU: LayerNorm / ResidualAddLayerNorm on every launch form, GELU / SiLU over every 16-bit bit
pattern, grid RoPE bit for bit against the golden.  Goldens are tests/dit_block_golden.py (pinned to the reference's recorded
outputs by tests/test_dit_block_golden.py), evaluated on the CPU; the ulp counts are against the same formulas in fp64.

Measured on MI355X (the figures the assertions below hold the kernels to; DESIGN 4.22 quotes them):
  * LayerNorm, 16-bit: see ``FAR_FROM_FP64`` (0 to 50 of 3.3 million elements per test further than one storage ulp from fp64,
    all where the result nearly cancels; torch's CPU kernel has 14 to 264 on the same inputs).
  * LayerNorm, fp32 rows at 1000 +- 1: 3.3e-7 (no affine) and 6.1e-7 (affine) from fp64 at dim 5120, where torch's CPU kernel is
    1.4e-4 off (affine; 4e-5 without) and so misses the reference's own 1e-4 bound -- that row is checked against fp64 only.
  * GELU / SiLU: within one storage ulp of fp64 on every finite bit pattern; see ``GOLDEN_DIFFERS`` for the count against torch
    (asserted not to grow).  Non-finite inputs give the golden's class: GELU of +-inf is NaN, as torch's.
  * grid RoPE: 0 elements differ from the CPU golden in bf16 and fp16.  In fp32 torch's complex product rounds differently in the
    remainder of its vector loop (112 of 10 800 and 37 of 220 elements differ on the two small cases, none on the three of the
    reference's test), so fp32 is held to the rounding bound of the formula against fp64.
"""
import pytest
import torch

import dit_block_golden as G
from conftest import bit_equal
from mojo_opset_amd.backends import hip
from mojo_opset_amd.backends.hip import lib as L
from mojo_opset_amd.backends.hip.operators import streaming as S

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = [pytest.param(BF16, id="bf16"), pytest.param(F16, id="fp16"), pytest.param(F32, id="fp32")]
ROWS = (1, 3, 257)
EPS = 1e-5


def wide(dtype):
    return 16 // torch.empty((), dtype=dtype).element_size()


def cached_dim(vec, tpr=256):
    """The longest row a launch form keeps in registers: the unit's table (`mojo_hip_layernorm_cache_vectors`)."""
    return vec * tpr * L.load().mojo_hip_layernorm_cache_vectors()


def ln_dims(dtype):
    """(dim, element offset of the base pointer).  The issue's dims, then per vector width the last dim the 256-thread form
    caches and the first it re-reads (a 2-element offset takes the 2-element vectors, an odd one single elements), then one
    dim well inside the re-read path."""
    w = wide(dtype)
    dims = [(d, 0) for d in (1, 2, 7, 8, 24, 40, 1000, 5120)]
    dims += [(cached_dim(w), 0), (cached_dim(w) + w, 0), (cached_dim(2), 2), (cached_dim(2) + 2, 2), (cached_dim(1), 1), (cached_dim(1) + 1, 1)]
    dims += [(w * 300, 0), (602, 0), (301, 0), (3 * cached_dim(1) + 5, 0)]          # two waves per row; the re-read path thrice over
    return dims


@pytest.fixture(scope="module")
def ln_data():
    """Per (dtype, dim): x, residual [257, dim], weight, bias, and the goldens of the four variants on all 257 rows -- computed
    once, shared, never written to."""
    cache = {}

    def get(dtype, dim):
        key = (dtype, dim)
        if key not in cache:
            g = torch.Generator().manual_seed(1000 + dim)
            x = (torch.randn(ROWS[-1], dim, generator=g) * 2 + 0.5).to(dtype)
            r = torch.randn(ROWS[-1], dim, generator=g).to(dtype)
            w = (torch.randn(dim, generator=g) * 0.5 + 1).to(dtype)
            b = torch.randn(dim, generator=g).to(dtype)
            s = x + r
            gold = {
                "affine": torch.nn.functional.layer_norm(x, (dim,), w, b, EPS),
                "plain": torch.nn.functional.layer_norm(x, (dim,), None, None, EPS),
                "sum": s,
                "residual": torch.nn.functional.layer_norm(s, (dim,), w, b, EPS),
            }
            f64 = {"affine": G.layernorm_fp64(x, w, b, EPS), "plain": G.layernorm_fp64(x, None, None, EPS),
                   "residual": G.layernorm_fp64(s, w, b, EPS)}
            cache[key] = (x, r, w, b, gold, f64)
        return cache[key]

    return get


def offset_copy(t, off, row_stride=None):
    """``t`` [rows, dim] on the device inside a larger buffer: the base ``off`` elements in, rows ``row_stride`` apart."""
    rows, dim = t.shape
    ld = row_stride or dim
    buf = torch.zeros(off + rows * ld + 8, dtype=t.dtype, device=DEV)
    view = buf[off:off + rows * ld].view(rows, ld)[:, :dim]
    view.copy_(t)
    return view


def make_norm(variant, dim, dtype, w, b):
    if variant in ("affine", "plain"):
        op = hip.HIPLayerNorm(dim, EPS, variant == "affine", dtype=dtype, device=DEV)
    else:
        op = hip.HIPResidualAddLayerNorm(dim, EPS, variant, dtype=dtype, device=DEV)
    if op.weight is not None:
        with torch.no_grad():
            op.weight.copy_(w)
            op.bias.copy_(b)
    return op


def norm_tolerance(dtype, variant):
    """The reference's own test tolerances: a ceiling."""
    if dtype != F32:
        return dict(atol=5e-2, rtol=1e-2)
    return dict(atol=1e-4, rtol=1e-5) if variant in ("affine", "plain") else dict(atol=1e-5, rtol=1e-6)


# Elements, summed over a test's dims and row counts (3.3 million per test), further than one storage ulp from the fp64 value of
# the same formula, measured on MI355X.  The issue expected 0; what remains sits where the result nearly cancels (x - mean, or
# y * w + b, within 1e-5 of zero): the result's ulp is then below the fp32 rounding of its terms (6e-8 of |mean| or |y * w|), which
# no fp32 evaluation can see.  torch's CPU result has 19 / 264 / 14 / 14 (bf16) and 33 / 255 / 36 / 36 (fp16) on the same inputs
# (printed beside the kernel's).  The assertion: the count does not grow.
FAR_FROM_FP64 = {(BF16, "affine"): 25, (BF16, "plain"): 21, (BF16, "pre"): 12, (BF16, "post"): 12,
                 (F16, "affine"): 50, (F16, "plain"): 0, (F16, "pre"): 41, (F16, "post"): 41}


def plain_forms(dtype):
    """Every launch form of the unit that a shape alone selects (the non-temporal ones follow the stream switch)."""
    return {f"layernorm:vec{vec}:{form}:plain" for vec in (wide(dtype), 2, 1)
            for form in ("tpr64:cached", "tpr128:cached", "tpr256:cached", "tpr256:reread")}


@pytest.mark.parametrize("variant", ["affine", "plain", "pre", "post"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_layernorm_matches_the_golden_on_every_dim_and_row_count(ln_data, dtype, variant):
    far, far_golden, taken = 0, 0, set()
    for dim, off in ln_dims(dtype):
        x, r, w, b, gold, f64 = ln_data(dtype, dim)
        op = make_norm(variant, dim, dtype, w, b)
        key = variant if variant in ("affine", "plain") else "residual"
        for rows in ROWS:
            xd = offset_copy(x[:rows], off)
            L.launch_history(clear=True)
            if key == "residual":
                normed, second = op(xd, offset_copy(r[:rows], off))
            else:
                normed, second = op(xd), None
            tag = L.last_launch()
            assert tag.startswith("layernorm:vec") and L.launch_history() == tag, tag
            taken.add(tag)
            assert normed.shape == (rows, dim) and normed.dtype == dtype and normed.is_contiguous()
            if variant == "pre":
                assert bit_equal(second, gold["sum"][:rows]), (dim, rows, tag)
            elif variant == "post":
                assert second is normed
            got = normed.cpu()
            torch.testing.assert_close(got, gold[key][:rows], **norm_tolerance(dtype, variant), msg=lambda m: f"dim {dim} rows {rows} {tag}: {m}")
            if dtype == F32:
                torch.testing.assert_close(got.double(), f64[key][:rows], **norm_tolerance(dtype, variant))
            else:
                far += int((G.ulp_distance(got, f64[key][:rows]) > 1).sum())
                far_golden += int((G.ulp_distance(gold[key][:rows], f64[key][:rows]) > 1).sum())
            if dim == 1:                                            # the variance is 0: the output is the bias, or 0
                assert torch.equal(got, (b if variant != "plain" else torch.zeros(1, dtype=dtype)).expand(rows, 1))
    assert taken == plain_forms(dtype), sorted(taken ^ plain_forms(dtype))           # every launch form was taken
    if dtype != F32:
        print(f"layernorm {dtype} {variant}: {far} elements further than one storage ulp from fp64 (torch on the CPU: {far_golden}; "
              f"recorded: {FAR_FROM_FP64[(dtype, variant)]})")
        assert far <= FAR_FROM_FP64[(dtype, variant)]


def test_layernorm_non_temporal_forms(ln_data, monkeypatch):
    """What the sweep above cannot reach by shape alone: the non-temporal forms of the 16-byte vectors, with the shared stream
    switch forced on."""
    monkeypatch.setenv("MOJO_HIP_STREAM_NT", "1")
    for dtype in (BF16, F16, F32):
        w_, taken = wide(dtype), set()
        for dim, rows in ((40, 257), (w_ * 300, 257), (cached_dim(w_), 3), (cached_dim(w_) + w_, 3)):
            x, r, w, b, gold, _ = ln_data(dtype, dim)
            normed, summed = make_norm("pre", dim, dtype, w, b)(x[:rows].to(DEV), r[:rows].to(DEV))
            taken.add(L.last_launch())
            assert bit_equal(summed, gold["sum"][:rows])
            torch.testing.assert_close(normed.cpu(), gold["residual"][:rows], **norm_tolerance(dtype, "pre"))
        assert taken == {f"layernorm:vec{w_}:{form}:nt" for form in ("tpr64:cached", "tpr128:cached", "tpr256:cached", "tpr256:reread")}, taken
        narrow = make_norm("plain", 7, dtype, None, None)(ln_data(dtype, 7)[0].to(DEV))      # the narrow forms have no such twin
        assert L.last_launch() == "layernorm:vec1:tpr64:cached:plain"
        torch.testing.assert_close(narrow.cpu(), ln_data(dtype, 7)[4]["plain"], **norm_tolerance(dtype, "plain"))


@pytest.mark.parametrize("dtype", DTYPES)
def test_layernorm_reads_row_strided_views_in_place(ln_data, dtype):
    """A column slice of a wider tensor (rows 5120 + 64 apart) and a [B, T, D] view of it: no copy, same bits as the dense call."""
    dim, rows = 5120, 6
    x, r, w, b, gold, _ = ln_data(dtype, dim)
    xd, rd = offset_copy(x[:rows], 0, dim + 64), offset_copy(r[:rows], 0, dim + 128)
    assert not xd.is_contiguous() and S._row_view(xd) == (rows, dim + 64)
    for variant in ("affine", "pre"):
        op = make_norm(variant, dim, dtype, w, b)
        dense = op(x[:rows].to(DEV)) if variant == "affine" else op(x[:rows].to(DEV), r[:rows].to(DEV))
        strided = op(xd) if variant == "affine" else op(xd, rd)
        assert bit_equal(strided, dense)
        three_d = op(xd.view(2, 3, dim)) if variant == "affine" else op(xd.view(2, 3, dim), rd.view(2, 3, dim))
        first = three_d if variant == "affine" else three_d[0]
        assert first.shape == (2, 3, dim) and bit_equal(first.view(rows, dim), dense if variant == "affine" else dense[0])
    odd = offset_copy(x[:rows], 1, dim + 3)                         # odd base, odd stride: single elements
    got = make_norm("plain", dim, dtype, w, b)(odd)
    assert L.last_launch().startswith("layernorm:vec1:")
    torch.testing.assert_close(got.cpu(), gold["plain"][:rows], **norm_tolerance(dtype, "plain"))
    transposed = x[:rows].to(DEV).t().contiguous().t()              # the last dimension is not dense: copied, still right
    torch.testing.assert_close(make_norm("plain", dim, dtype, w, b)(transposed).cpu(), gold["plain"][:rows], **norm_tolerance(dtype, "plain"))


def test_layernorm_of_a_row_far_from_zero_keeps_its_digits():
    """fp32 rows with mean 1000 and unit spread: E[x^2] - mean^2 would lose every digit (1e6 against 1, in a 24-bit
    significand); the centred form meets the plain op's bound against fp64, affine or not, cached or re-read."""
    for dim in (5120, 3 * cached_dim(4) + 4):
        g = torch.Generator().manual_seed(dim)
        x = 1000 + torch.randn(3, dim, generator=g)
        w, b = torch.randn(dim, generator=g), torch.randn(dim, generator=g)
        for affine in (False, True):
            got = make_norm("affine" if affine else "plain", dim, F32, w, b)(x.to(DEV)).cpu()
            want = G.layernorm_fp64(x, w if affine else None, b if affine else None, EPS)
            err = (got.double() - want).abs().max().item()
            print(f"mean-1000 rows, dim {dim}, affine {affine}: max abs error {err:.3g}")
            torch.testing.assert_close(got.double(), want, atol=1e-4, rtol=1e-5)
            # (torch's CPU kernel is itself 1.4e-4 from fp64 on these rows, outside this bound: printed, not a yardstick here)
            cpu = torch.nn.functional.layer_norm(x, (dim,), w if affine else None, b if affine else None, EPS)
            print(f"    torch on the CPU: max abs error {(cpu.double() - want).abs().max().item():.3g}")


def test_norms_return_without_a_launch_on_empty_input():
    L.launch_history(clear=True)
    ln = hip.HIPLayerNorm(8, dtype=BF16, device=DEV)
    assert ln(torch.empty(0, 8, dtype=BF16, device=DEV)).shape == (0, 8)
    ra = hip.HIPResidualAddLayerNorm(8, dtype=BF16, device=DEV)
    normed, summed = ra(torch.empty(2, 0, 8, dtype=BF16, device=DEV), torch.empty(2, 0, 8, dtype=BF16, device=DEV))
    assert normed.shape == summed.shape == (2, 0, 8)
    for op in (hip.HIPGelu(), hip.HIPSilu()):
        assert op(torch.empty(0, 3, dtype=F16, device=DEV)).shape == (0, 3)
    rope = hip.HIPGridRoPE()
    out = rope(torch.empty(0, 4, 2, 8, dtype=BF16, device=DEV), torch.empty(0, 3, dtype=torch.int32, device=DEV), [])
    assert out.shape == (0, 4, 2, 8)
    assert L.launch_history() == ""


# ---- GELU / SiLU -------------------------------------------------------------------------------------------------------------
ACTS = {"gelu": (hip.HIPGelu, G.TorchGelu, G.gelu_fp64, "gelu_erf"), "silu": (hip.HIPSilu, G.TorchSilu, G.silu_fp64, "silu")}
# Elements (of the 65 536 bit patterns) whose result differs at all from torch's CPU result, measured on MI355X.  torch
# evaluates 1 + erf(z) and x / (1 + exp(-x)) in fp32 and flushes subnormals; the kernel is held to the fp64 value instead, so
# these are torch's departures from it, not the kernel's.  The assertion: the count does not grow.
GOLDEN_DIFFERS = {("gelu", BF16): 848, ("gelu", F16): 577, ("silu", BF16): 18, ("silu", F16): 1}


def all_patterns(dtype):
    return torch.arange(1 << 16, dtype=torch.int32).to(torch.int16).view(dtype)


@pytest.mark.parametrize("dtype", DTYPES[:2])
@pytest.mark.parametrize("act", ["gelu", "silu"])
def test_activation_on_every_bit_pattern(act, dtype):
    hip_cls, torch_cls, fp64, tag = ACTS[act]
    x = all_patterns(dtype)
    gold, want = torch_cls().forward(x), fp64(x)
    finite = torch.isfinite(x.float())
    buf = torch.zeros((1 << 16) + 16, dtype=dtype, device=DEV)
    outs = {}
    # one aligned tensor; the same with 5 more elements (a scalar tail); from an odd offset (single elements)
    for name, lo, n, vec in (("aligned", 0, 1 << 16, 8), ("tail", 0, (1 << 16) + 5, 8), ("odd", 1, 1 << 16, 1)):
        buf.zero_()
        buf[lo:lo + (1 << 16)].copy_(x)
        L.launch_history(clear=True)
        out = hip_cls()(buf[lo:lo + n])
        assert L.launch_history() == f"activation:{tag}:vec{vec}:plain"
        assert out.shape == (n,) and out.dtype == dtype
        if n > 1 << 16:
            assert bool((out[1 << 16:].float() == 0).all())          # f(0) = 0
        outs[name] = out[:1 << 16].cpu()
    got = outs["aligned"]
    assert bit_equal(outs["tail"], got) and bit_equal(outs["odd"], got)
    # finite inputs: within one storage ulp of the fp64 value rounded once
    assert bool(torch.isfinite(got[finite].float()).all())
    dist = G.ulp_distance(got[finite], want[finite])
    print(f"{act} {dtype}: max ulp distance from fp64 {int(dist.max())}, {int((dist > 0).sum())} of {int(finite.sum())} not the nearest")
    assert int(dist.max()) <= 1
    # non-finite inputs: the golden's class
    gn, on = gold[~finite].float(), got[~finite].float()
    assert torch.equal(torch.isnan(gn), torch.isnan(on))
    rest = ~torch.isnan(gn)
    assert torch.equal(gn[rest], on[rest]) and torch.equal(torch.signbit(gn[rest]), torch.signbit(on[rest]))
    # against torch's CPU result at all
    differs = int((got[finite].view(torch.int16) != gold[finite].view(torch.int16)).sum())
    print(f"{act} {dtype}: {differs} of {int(finite.sum())} finite inputs differ from the CPU golden (recorded: {GOLDEN_DIFFERS[(act, dtype)]})")
    assert GOLDEN_DIFFERS[(act, dtype)] is not None and differs <= GOLDEN_DIFFERS[(act, dtype)]
    # in place: out is in
    xd = x.to(DEV)
    assert S._activation(act, xd, S.ACT_GELU_ERF if act == "gelu" else S.ACT_SILU, out=xd) is xd
    assert bit_equal(xd, got)


@pytest.mark.parametrize("act", ["gelu", "silu"])
def test_activation_fp32(act):
    hip_cls, torch_cls, fp64, tag = ACTS[act]
    g = torch.Generator().manual_seed(9)
    x = torch.cat([torch.randn(1 << 16, generator=g) * 4, torch.tensor([0.0, -0.0, 1e-30, -1e-30, 88.0, -88.0, 1e4, -1e4])])
    got = hip_cls()(x.to(DEV))
    assert L.last_launch() == f"activation:{tag}:vec4:plain"
    torch.testing.assert_close(got.cpu(), fp64(x).float())
    assert torch.equal(torch.signbit(got.cpu()[-8:]), torch.signbit(fp64(x).float()[-8:]))      # -0 stays -0
    shaped = x[:4096].view(4, 32, 32).to(DEV)
    assert bit_equal(hip_cls()(shaped.transpose(0, 2)), hip_cls()(shaped).transpose(0, 2))      # copied once, same values
    xd = x.to(DEV)
    S._activation(act, xd, S.ACT_GELU_ERF if act == "gelu" else S.ACT_SILU, out=xd)
    assert bit_equal(xd, got)


def test_activation_non_temporal_form_gives_the_same_bits(monkeypatch):
    x = all_patterns(BF16).to(DEV)
    plain = {act: ACTS[act][0]()(x) for act in ACTS}
    monkeypatch.setenv("MOJO_HIP_STREAM_NT", "1")
    for act in ACTS:
        assert bit_equal(ACTS[act][0]()(x), plain[act]) and L.last_launch() == f"activation:{ACTS[act][3]}:vec8:nt"


# ---- grid RoPE ---------------------------------------------------------------------------------------------------------------
def frequencies(cells, head_dim):
    inv_freq = 1.0 / (10000.0 ** (torch.arange(0, head_dim, 2, dtype=F32) / head_dim))
    angle = torch.arange(cells, dtype=F32)[:, None] * inv_freq[None, :]
    return torch.complex(angle.cos()[:, None, :], angle.sin()[:, None, :])


def rope_case(grids, pad, heads, head_dim, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    cells = [f * h * w for f, h, w in grids]
    x = torch.randn(len(grids), max(cells) + pad, heads, head_dim, generator=g).to(dtype)
    return x, torch.tensor(grids, dtype=torch.int32), cells


ROPE_CASES = [
    # (grids, padding behind the largest, heads, head_dim): the reference's three, then per-sample grids (one filling L exactly,
    # one of a single cell) and D = 2
    pytest.param([(2, 4, 8)] * 4, 10, 8, 64, id="ref-4x64"), pytest.param([(1, 8, 8)] * 2, 5, 16, 128, id="ref-2x128"),
    pytest.param([(4, 4, 4)] * 3, 3, 4, 64, id="ref-3x64"), pytest.param([(2, 3, 5), (1, 1, 1), (3, 2, 2)], 0, 3, 40, id="per-sample"),
    pytest.param([(1, 3, 3), (2, 2, 2)], 2, 5, 2, id="d2"),
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("grids, pad, heads, head_dim", ROPE_CASES)
def test_grid_rope_equals_the_golden_bit_for_bit(grids, pad, heads, head_dim, dtype):
    x, grid, cells = rope_case(grids, pad, heads, head_dim, dtype)
    same = len(set(cells)) == 1
    distinct = [frequencies(c, head_dim) for c in cells]
    gold = G.TorchGridRoPE().forward(x, grid, distinct)
    op = hip.HIPGridRoPE()
    got = op(x.to(DEV), grid.to(DEV), [f.to(DEV) for f in distinct])              # a list of distinct tensors: packed
    assert L.last_launch().startswith("grid_rope:vec")
    assert got.shape == x.shape and got.dtype == dtype and got.is_contiguous()
    differs = int((got.cpu() != gold).sum())
    print(f"grid rope {dtype} D={head_dim}: {differs} of {gold.numel()} differ from the CPU golden")
    for i, c in enumerate(cells):                                                 # padding tokens: the input's bits
        assert bit_equal(got[i, c:], x[i, c:])
    if dtype == F32:
        # torch's CPU complex product rounds differently in the remainder of its vector loop, so fp32 has no bit-exact golden:
        # the reference's 1e-3 is the ceiling, the formula's own rounding (two products and a sum, 3 x 2^-24 of |a| + |b|) the bound
        torch.testing.assert_close(got.cpu(), gold, atol=1e-3, rtol=1e-3)
        mag = x.double().abs().unflatten(-1, (-1, 2)).sum(-1, keepdim=True).expand(-1, -1, -1, -1, 2).flatten(-2)
        assert bool(((got.cpu().double() - G.grid_rope_fp64(x, grid, distinct)).abs() <= 3 * 2.0 ** -24 * mag).all())
        return
    assert bit_equal(got, gold)
    assert int(G.ulp_distance(got.cpu(), G.grid_rope_fp64(x, grid, distinct)).max()) <= 1
    if same:                                                                      # one shared tensor: one pointer, same bits
        shared = distinct[0].to(DEV)
        assert bit_equal(op(x.to(DEV), grid.to(DEV), [shared] * len(cells)), gold)
    # grid_sizes on the CPU (checked on the host) and as int64 on the device
    assert bit_equal(op(x.to(DEV), grid, [f.to(DEV) for f in distinct]), gold)
    assert bit_equal(op(x.to(DEV), grid.long().to(DEV), [f.to(DEV) for f in distinct]), gold)


@pytest.mark.parametrize("dtype", DTYPES[:2])
def test_grid_rope_reads_a_slice_of_a_fused_qkv_buffer_in_place(dtype):
    grids, heads, head_dim = [(2, 3, 4), (1, 5, 4)], 6, 64
    g = torch.Generator().manual_seed(3)
    tokens = 27
    qkv = torch.randn(2, tokens, 3, heads, head_dim, generator=g).to(dtype)
    grid = torch.tensor(grids, dtype=torch.int32)
    freqs = [frequencies(f * h * w, head_dim) for f, h, w in grids]
    dev = qkv.to(DEV)
    op = hip.HIPGridRoPE()
    for which in (0, 1):
        x = dev[:, :, which]
        assert not x.is_contiguous() and x.stride() == (tokens * 3 * heads * head_dim, 3 * heads * head_dim, head_dim, 1)
        got = op(x, grid.to(DEV), [f.to(DEV) for f in freqs])
        assert L.last_launch() == f"grid_rope:vec{wide(dtype)}:plain"
        assert bit_equal(got, G.TorchGridRoPE().forward(qkv[:, :, which], grid, freqs))
    assert bit_equal(dev, qkv)                                                    # the buffer itself is untouched
    odd = dev[:, :, 0, :, 2:]                                                     # D = 62 from a 4-byte-aligned base: pairs
    got = op(odd, grid.to(DEV), [f[..., 1:].contiguous().to(DEV) for f in freqs])
    assert L.last_launch() == "grid_rope:vec2:plain"
    assert bit_equal(got, G.TorchGridRoPE().forward(qkv[:, :, 0, :, 2:], grid, [f[..., 1:] for f in freqs]))


def test_grid_rope_is_exact_on_exact_inputs():
    """Small integers times (1, 0), (0, 1), (-1, 0): every product and sum is exact in every format, so a swapped pair or a
    wrong sign cannot hide in a tolerance.  (a + ib) * 1 = (a, b); * i = (-b, a); * -1 = (-a, -b)."""
    heads, head_dim, cells, tokens = 3, 8, 12, 14
    g = torch.Generator().manual_seed(5)
    xi = torch.randint(-8, 9, (2, tokens, heads, head_dim), generator=g)
    which = torch.randint(0, 3, (cells, 1, head_dim // 2), generator=g)
    freqs = torch.complex(torch.tensor([1.0, 0.0, -1.0])[which], torch.tensor([0.0, 1.0, 0.0])[which])
    a, b = xi[..., 0::2], xi[..., 1::2]
    k = which[None].expand(2, cells, heads, head_dim // 2)
    re = torch.where(k == 0, a[:, :cells], torch.where(k == 1, -b[:, :cells], -a[:, :cells]))
    im = torch.where(k == 0, b[:, :cells], torch.where(k == 1, a[:, :cells], -b[:, :cells]))
    want = xi.clone()
    want[:, :cells, :, 0::2], want[:, :cells, :, 1::2] = re, im
    grid = torch.tensor([[2, 3, 2], [1, 4, 3]], dtype=torch.int32, device=DEV)
    for dtype in (BF16, F16, F32):
        got = hip.HIPGridRoPE()(xi.to(dtype).to(DEV), grid, [freqs.to(DEV)] * 2)
        assert torch.equal(got.cpu().long(), want), dtype
        assert bit_equal(G.TorchGridRoPE().forward(xi.to(dtype), grid.cpu(), [freqs] * 2), want.to(dtype))


def test_grid_rope_never_reads_past_a_frequency_entry():
    """grid_sizes on the device names more cells than an entry has rows (the caller's error, documented): the tokens the
    entry covers are rotated, the rest copied; the rows of the NEXT entry in the packed buffer are not used for them."""
    heads, head_dim = 2, 16
    x, _, _ = rope_case([(1, 2, 5), (1, 2, 5)], 0, heads, head_dim, BF16)
    freqs = [frequencies(6, head_dim), frequencies(10, head_dim) * torch.complex(torch.tensor(0.0), torch.tensor(1.0))]
    grid = torch.tensor([[1, 2, 5], [1, 2, 5]], dtype=torch.int32)
    got = hip.HIPGridRoPE()(x.to(DEV), grid.to(DEV), [f.to(DEV) for f in freqs])
    honest = G.TorchGridRoPE().forward(x, torch.tensor([[1, 2, 3], [1, 2, 5]], dtype=torch.int32), freqs)
    assert bit_equal(got, honest)
    with pytest.raises(ValueError, match="10 cells"):
        hip.HIPGridRoPE()(x.to(DEV), grid, [f.to(DEV) for f in freqs])              # on the CPU the same grid is refused


def test_grid_rope_non_temporal_form_gives_the_same_bits(monkeypatch):
    x, grid, cells = rope_case([(2, 4, 8)] * 2, 3, 4, 128, BF16)
    freqs = [frequencies(cells[0], 128).to(DEV)] * 2
    plain = hip.HIPGridRoPE()(x.to(DEV), grid.to(DEV), freqs)
    monkeypatch.setenv("MOJO_HIP_STREAM_NT", "1")
    assert bit_equal(hip.HIPGridRoPE()(x.to(DEV), grid.to(DEV), freqs), plain) and L.last_launch() == "grid_rope:vec8:nt"
