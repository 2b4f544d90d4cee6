"""Inputs and float64 restatements shared by tests/test_quant_dense_golden.py (CPU) and tests/test_hip_quant_dense.py (GPU):
the GPU tests compare the hip backend with the fp32 golden at a bound of one quantisation step on at most 2e-3 of the elements;
the CPU test shows that these very inputs leave room for that bound (the golden against statistics, or silu, computed in
float64 differs on at most a tenth of it)."""
import functools

import torch

import quant_dense_golden as G

BF16, F16, F32, I8, F8 = torch.bfloat16, torch.float16, torch.float32, torch.int8, torch.float8_e4m3fn

# rows x dim of the reference-space sweep: 20000 exceeds the register cache; 257 and 1000 have no 16-byte vectors
SWEEP_SHAPES = [(1, 128), (7, 257), (5, 1000), (32, 1024), (3, 20000), (64, 8192)]
NORM_DTYPES = [F16, BF16, F32]
# (tokens, H, token_count or None): H 14400 exceeds the register cache (14336 columns); 257 has no 16-byte vectors
SWIGLU_SWEEP = [(12, 64, [4, 3, 5]), (9, 257, None), (30, 512, [6, 3, 8, 5, 8]), (40, 1000, [0, 25, 0, 15]), (33, 4096, [20, 13]),
                (3, 14400, None)]


@functools.lru_cache(None)
def norm_inputs(shape, dtype):
    """(x, residual, weight, bias, smooth): random-normal activations of ``dtype``, fp32 per-column vectors."""
    g = torch.Generator().manual_seed(shape[0] * 131 + shape[-1])
    x, r = torch.randn(shape, generator=g).to(dtype), torch.randn(shape, generator=g).to(dtype)
    dim = shape[-1]
    return x, r, torch.randn(dim, generator=g), torch.randn(dim, generator=g), torch.rand(dim, generator=g) + 0.5


@functools.lru_cache(None)
def swiglu_inputs(tokens, hidden, counts):
    """(accumulators int32 [T, 2H], activation_scale [T], weight_scale [E, 2H], quant_scale [E, H], bias [E, 2H], token_count):
    |acc| up to 2^14, per-token scales around 0.2, per-column scales around 0.005: gate values of a few units."""
    experts = 1 if counts is None else len(counts)
    g = torch.Generator().manual_seed(tokens * 131 + hidden)
    acc = (torch.randn(tokens, 2 * hidden, generator=g) * 3000).round().clamp(-2 ** 14, 2 ** 14).to(torch.int32)
    act = torch.rand(tokens, generator=g) * 0.3 + 0.05
    ws = torch.rand(experts, 2 * hidden, generator=g) * 0.008 + 0.001
    qs = torch.rand(experts, hidden, generator=g) + 0.5
    bias = torch.randn(experts, 2 * hidden, generator=g) * 0.1
    token_count = None if counts is None else torch.tensor(counts, dtype=torch.int64)
    return acc, act, ws, qs, bias, token_count


def make_op(cls, state=None, device=None, **kwargs):
    """``cls(**kwargs)`` with the parameters named in ``state`` set (and moved to ``device``)."""
    op = cls(**kwargs)
    with torch.no_grad():
        for name, value in (state or {}).items():
            getattr(op, name).copy_(value)
    return op if device is None else op.to(device)


def quantise_rows(y, q_min, q_max, quant_dtype):
    scale = y.abs().amax(dim=-1, keepdim=True).clamp(min=1e-12) / q_max
    return torch.clamp(torch.round(y / scale), q_min, q_max).to(quant_dtype), scale


def _fma(a, b, c):
    """fp32 fma of fp32 tensors (the product of two fp32 values is exact in float64)."""
    return (a.double() * b.double() + c.double()).float()


def layernorm_quant_f64(x, weight, bias, smooth, eps, q_min, q_max, quant_dtype):
    """`TorchLayerNormQuant` with mean and rstd computed in float64 and rounded to fp32; the elementwise part in fp32, in the
    form that reproduces torch's CPU layer_norm bit for bit: fma((x - mean) * rstd, w, b)."""
    xf = x.float()
    mean = xf.double().mean(dim=-1, keepdim=True)
    var = ((xf.double() - mean) ** 2).mean(dim=-1, keepdim=True)
    rstd = (1.0 / torch.sqrt(var + eps)).float()
    y = (xf - mean.float()) * rstd
    if weight is not None:
        y = _fma(y, weight.float().expand_as(y), bias.float().expand_as(y))
    if smooth is not None:
        y = y * smooth.float()
    return quantise_rows(y, q_min, q_max, quant_dtype)


def rmsnorm_quant_f64(x, weight, smooth, eps, q_min, q_max, quant_dtype):
    xf = x.float()
    rstd = torch.rsqrt((xf.double() ** 2).mean(dim=-1, keepdim=True) + eps).float()
    y = xf * rstd * weight.float()
    if smooth is not None:
        y = y * smooth.float()
    return quantise_rows(y, q_min, q_max, quant_dtype)


def swiglu_quant_f64(x, act, ws, qs, bias, token_count, activate_left):
    """`TorchDequantSwiGLUQuant` with silu evaluated in float64 and rounded to fp32; everything else as the golden."""
    tokens = x.shape[0]
    if token_count is None:
        expert = torch.zeros(tokens, dtype=torch.long)
    else:
        ends = token_count.to(torch.long).clamp(min=0).cumsum(0).clamp(max=tokens)
        assert int(ends[-1]) == tokens
        expert = torch.searchsorted(ends, torch.arange(tokens), right=True)
    y = x.float() * ws.float()[expert]
    if act is not None:
        y = y * act.float().unsqueeze(-1)
    if bias is not None:
        y = y + (bias.float()[expert] if bias.dim() == 2 else bias.float())
    left, right = y.chunk(2, dim=-1)
    gate, up = (left, right) if activate_left else (right, left)
    silu = (gate.double() / (1.0 + torch.exp(-gate.double()))).float()
    return quantise_rows(silu * up * qs.float()[expert], -128, 127, I8)


def q_difference(q, want_q):
    """(largest difference of the quantised values, share of elements that differ)."""
    diff = (q.float() - want_q.float()).abs()
    return float(diff.max()), float((diff > 0).float().mean())


def scale_rel_error(scale, want_scale):
    return float(((scale.double() - want_scale.double()).abs() / want_scale.double().abs()).max())


def golden_cls(name):
    return getattr(G, "Torch" + name[4:])


def norm_tie_case(name, quant_dtype, symmetric, dtype):
    """(state, constructor keywords, forward arguments, expected q) of a norm+quant op on rows whose normalisation is exact:
    x = +-1 alternating and eps = 0 give mean 0, variance and mean square 1 and rstd 1 in any summation order, so y = x * w, and w
    puts y / scale exactly on k + 0.5 for every k of the range, with scale = 2^-4 (one column carries q_max * 2^-4).  The
    residual-add op gets x as +-0.5 + +-0.5 (an exact sum)."""
    rows, dim = 6, 1024
    q_max = 127 if quant_dtype == I8 else 448
    q_min = (-128 if symmetric else 0) if quant_dtype == I8 else -448
    sign = torch.where(torch.arange(dim) % 2 == 0, 1.0, -1.0)
    ties = (torch.arange(dim) % (2 * q_max) - q_max).float() + 0.5            # |k + 0.5| < q_max, both signs
    ties[5] = q_max                                                          # the row maximum: scale = 2^-4 exactly
    w = ties * 2.0 ** -4 * sign
    x = sign.repeat(rows, 1)
    x[1::2] *= -1                                                            # odd rows: y = -ties
    y_over_scale = (x * w) * 16
    expected = torch.clamp(torch.round(y_over_scale), q_min, q_max).to(quant_dtype)
    state = {"weight": w} if name == "MojoRMSNormQuant" else {"weight": w, "bias": torch.zeros(dim)}
    kw = {"eps": 0.0, "quant_dtype": quant_dtype, "symmetric": symmetric}
    xs = x.to(dtype)
    args = (xs / 2, xs / 2) if name == "MojoResidualAddLayerNormQuant" else (xs,)
    return state, kw, args, expected
