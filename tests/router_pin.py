"""Which experts did the MoE router choose?  The host-side rule of DESIGN §4.21 (plain torch, no GPU).

`mojo_hip_moe_gating` has four routes (general streaming kernel, eight-expert stream, few-token pair, matrix cores) that share
`gate_softmax_topk`, whose documented order is "descending value, ties -> lowest expert id".  Two kinds of input pin it:

* exact cases (`exact_router_case`): data whose logits are exact in fp32 in ANY summation order and on the matrix-core route
  (the weights are exactly representable in bf16 / fp16, so the `lo` half of the split is zero), with a quarter of the expert
  columns exact copies of another column.  Every slot of every token must equal `expected_choice`, ties included.
* random cases (`random_router_case`): continuous data, where a kernel may differ from the fp64 choice only on tokens that
  `excused` holds for, under a margin `delta` taken from the REFERENCE's arithmetic (`deltas`), never from the kernel.

`well_formed` holds for every token, excused or not: a forgiven slot still feeds `moe_dispatch` as an index.

The tables below list the shapes of both test modules (tests/test_router_pin_golden.py on the host against the torch oracle,
tests/test_hip_moe_router.py on the device) with the launch tag each must report."""
import functools
from types import SimpleNamespace

import torch

GATE_ATOL, GATE_RTOL = 1e-5, 1e-4        # the suite's bound on a gate (tests/test_hip_moe.py)
LOGIT_SPREAD = 60.0                      # exp(-60) = 8.8e-27 is a normal fp32 number: order by probability == order by logit
DIFFERING_SHARE = 1e-3                   # random data: share of tokens that may differ from the fp64 choice (all of them excused)


# ---------------------------------------------------------------------------------------------------------------------------------
# exact cases
# ---------------------------------------------------------------------------------------------------------------------------------
def copy_pairs(experts, seed):
    """(source, copy) expert columns, about a quarter of the columns being copies, no column in two pairs.  The candidates
    rotate through: the 256-column edge (the GEMM's column tile, the few-token kernel's 256-expert chunk), the same lane of
    `gate_softmax_topk` in another register slot (e, e + 64 i), another 16-expert group (the few-token kernel's smallest
    `ep`), neighbouring lanes; random pairs fill up."""
    want = experts // 4
    groups = []
    if experts > 256:
        groups.append([(255, 256), (250, 260)] + [(e, e + 256) for e in range(3, experts - 256, 37)])
    if experts > 64:
        groups.append([(e, e + 64 * (1 + n % ((experts - 1 - e) // 64))) for n, e in enumerate(range(0, experts - 64, 9))])
    groups.append([(e, e + 16) for e in range(5, experts - 16, 23)])
    groups.append([(e, e + 1 + 2 * (n % 2)) for n, e in enumerate(range(1, experts - 3, 11))])
    gen = torch.Generator().manual_seed(seed)
    fill = torch.randint(0, experts, (8 * want + 8, 2), generator=gen).tolist() if experts > 1 else []
    groups.append([(s, d) for s, d in fill if s != d])
    used, pairs = set(), []
    at = [0] * len(groups)
    while len(pairs) < want and any(a < len(g) for a, g in zip(at, groups)):
        for gi, g in enumerate(groups):
            if at[gi] < len(g) and len(pairs) < want:
                s, d = g[at[gi]]
                at[gi] += 1
                if s not in used and d not in used:
                    used.update((s, d))
                    pairs.append((s, d))
    return pairs


@functools.lru_cache(maxsize=None)
def _exact_case(experts, k, hidden, tokens, seed, dense):
    gen = torch.Generator().manual_seed(seed)
    if dense:
        # weights: multiples of 2^-6 in [-1/4, 1/4]; activations in {-1, 0, 1}, about min(2/3 H, 512) non-zeros per token: a
        # logit is a multiple of 2^-6 below 2^11, every partial sum of it in any order too -> exact in fp32
        w = torch.randint(-16, 17, (hidden, experts), generator=gen).double() / 64
        density = min(2.0 / 3.0, 512.0 / hidden)
        x = (torch.rand(tokens, hidden, generator=gen) < density).double() * (torch.randint(0, 2, (tokens, hidden), generator=gen) * 2 - 1)
        x[tokens - 1, 0], x[tokens - 1, hidden - 1] = -1.0, -1.0
        x[0, 0], x[0, hidden - 1] = 1.0, -1.0
        unit = 64
    else:
        # at most four non-zeros (+-1, +-2) per token, weights multiples of 1/8 in [-2, 2]: one dropped or doubled hidden
        # position moves a logit by a whole multiple of 1/8
        w = torch.randint(-16, 17, (hidden, experts), generator=gen).double() / 8
        pos = torch.randint(0, hidden, (tokens, 4), generator=gen)
        pos[0, 0], pos[0, 1], pos[tokens - 1, 2] = 0, hidden - 1, hidden - 1
        val = (torch.randint(1, 3, (tokens, 4), generator=gen) * (torch.randint(0, 2, (tokens, 4), generator=gen) * 2 - 1)).double()
        x = torch.zeros(tokens, hidden, dtype=torch.float64)
        for j in range(4):                                           # a repeated position keeps its last value
            x[torch.arange(tokens), pos[:, j]] = val[:, j]
        unit = 8
    assert x[0, 0] != 0 and x[0, hidden - 1] != 0 and x[tokens - 1, hidden - 1] != 0
    pairs = copy_pairs(experts, seed + 1)
    for s, d in pairs:
        w[:, d] = w[:, s]
    logits = x @ w
    assert torch.equal(logits * unit, (logits * unit).round()) and float(logits.abs().max()) * unit < 2 ** 23      # exact in fp32
    assert float((logits.max(-1, keepdim=True).values - logits).max()) <= LOGIT_SPREAD                                # no underflow
    assert torch.equal((x.float() @ w.float()).double(), logits)                                                    # the reference's product too
    return SimpleNamespace(experts=experts, k=k, hidden=hidden, tokens=tokens, x64=x, w=w.float(), logits64=logits, pairs=pairs,
                           unit=unit)


def exact_router_case(experts, k, hidden, tokens, dtype, seed, dense):
    """Activations `x` [tokens, hidden] in `dtype`, gate weight `w` [hidden, experts] in fp32, and `logits64`, their product,
    which every route must reproduce bit for bit (asserted here on the host: exact in fp32, within 60 of the row maximum,
    distinct values >= 2^-6 apart because all are multiples of 1 / `unit`)."""
    c = _exact_case(experts, k, hidden, tokens, seed, bool(dense))
    x = c.x64.to(dtype)
    assert torch.equal(x.double(), c.x64) and torch.equal(c.w.to(dtype).float(), c.w)      # so w_lo == 0 on the matrix-core route
    return SimpleNamespace(**{**vars(c), "x": x, "dtype": dtype})


def tie_profile(logits64, k):
    """(tokens with a tie inside the first k places, tokens whose k-th and (k+1)-th logits tie) — what the copies are for."""
    s = torch.sort(logits64, dim=-1, descending=True).values
    inside = (s[:, : k - 1] == s[:, 1:k]).any(-1) if k > 1 else torch.zeros(s.shape[0], dtype=torch.bool)
    across = s[:, k - 1] == s[:, k] if k < s.shape[1] else torch.zeros(s.shape[0], dtype=torch.bool)
    return inside, across


# ---------------------------------------------------------------------------------------------------------------------------------
# the rule
# ---------------------------------------------------------------------------------------------------------------------------------
def expected_choice(logits64, k):
    """The kernel's documented order: descending logit, ties -> lowest expert id.  Returns (ids int32 [T, k], gates fp64 [T, k])."""
    order = torch.sort(-logits64, dim=-1, stable=True).indices[:, :k]
    return order.to(torch.int32), chosen_gates(logits64, order)


def chosen_gates(logits64, idx):
    """softmax over all experts, renormalised over the chosen == softmax over the chosen logits (fp64)."""
    return torch.softmax(torch.gather(logits64, 1, idx.to(torch.int64)), dim=-1)


def tie_free(logits64, k):
    """Tokens without a tie inside the first k + 1 places: where `torch.topk`, which leaves tie order open, is comparable."""
    s = torch.sort(logits64, dim=-1, descending=True).values[:, : k + 1]
    return ~(s[:, :-1] == s[:, 1:]).any(-1)


def well_formed(idx, gates, experts):
    """Per token: ids in [0, E) and distinct; gates finite, in (0, 1], non-increasing along k, summing to 1 within 1e-5.
    The dtypes (int32 ids, fp32 gates) are the whole result's and raise."""
    assert idx.dtype == torch.int32 and gates.dtype == torch.float32, (idx.dtype, gates.dtype)
    assert idx.shape == gates.shape and idx.dim() == 2
    ids = idx.to(torch.int64)
    ok = ((ids >= 0) & (ids < experts)).all(-1)
    s = torch.sort(ids, dim=-1).values
    ok &= (s[:, 1:] != s[:, :-1]).all(-1)
    g = gates.double()
    ok &= torch.isfinite(g).all(-1) & (g > 0).all(-1) & (g <= 1).all(-1)
    ok &= (g[:, 1:] <= g[:, :-1]).all(-1)
    ok &= (g.sum(-1) - 1).abs() <= 1e-5
    return ok


def shortfall(idx, logits64, k):
    """Per token (ids must be in range): how far the choice is from a valid one, in logit units — the larger of (k-th largest
    fp64 logit - smallest chosen logit) and the largest inversion between adjacent chosen logits.  0 for `expected_choice`."""
    chosen = torch.gather(logits64, 1, idx.to(torch.int64))
    kth = torch.sort(logits64, dim=-1, descending=True).values[:, k - 1]
    miss = (kth.unsqueeze(-1) - chosen).max(-1).values
    if k > 1:
        miss = torch.maximum(miss, (chosen[:, 1:] - chosen[:, :-1]).max(-1).values)
    return miss.clamp_min(0)


def excused(idx, gates, logits64, k, delta):
    """Per token: every chosen expert within `delta` of the k-th place, adjacent chosen logits inverted by at most `delta`,
    and the gates the softmax of the CHOSEN fp64 logits within 1e-5 / 1e-4."""
    ids = idx.to(torch.int64)
    in_range = ((ids >= 0) & (ids < logits64.shape[1])).all(-1)
    ids = ids.clamp(0, logits64.shape[1] - 1)
    want = chosen_gates(logits64, ids)
    gate_ok = ((gates.double() - want).abs() <= GATE_ATOL + GATE_RTOL * want.abs()).all(-1)
    return in_range & (shortfall(ids, logits64, k) <= delta) & gate_ok


def differing(idx, logits64, k):
    """Tokens whose ids differ from `expected_choice` in any slot."""
    return (idx != expected_choice(logits64, k)[0]).any(-1)


def deltas(x, w):
    """(delta_vec, delta_mfma, logits64) from the reference's own arithmetic: 8 x the largest error of the fp32 CPU product
    against the fp64 one (a different summation order errs by the same statistical size), and for the matrix-core route
    that plus the kernel's stated split accuracy, 2^-16 max_e |x o w_e|_2."""
    logits64 = x.double() @ w.double()
    delta_vec = 8.0 * float(((x.float() @ w).double() - logits64).abs().max())
    delta_mfma = delta_vec + 2.0 ** -16 * float(((x.double() ** 2) @ (w.double() ** 2)).max().sqrt())
    return delta_vec, delta_mfma, logits64


@functools.lru_cache(maxsize=None)
def random_router_case(experts, k, hidden, tokens, dtype, std, seed):
    """The suite's random data (tests/test_hip_moe.py): N(0, std) fp32 weights, `torch.rand` activations in `dtype`."""
    gen = torch.Generator().manual_seed(seed)
    w = torch.randn(hidden, experts, generator=gen) * std
    x = torch.rand(tokens, hidden, generator=gen).to(dtype)
    delta_vec, delta_mfma, logits64 = deltas(x, w)
    return SimpleNamespace(experts=experts, k=k, hidden=hidden, tokens=tokens, dtype=dtype, x=x, w=w, logits64=logits64,
                           delta_vec=delta_vec, delta_mfma=delta_mfma)


def judge_random(idx, gates, case, delta):
    """Asserts the random-data rule on one result; returns (differing tokens, largest shortfall among them / delta)."""
    assert bool(well_formed(idx, gates, case.experts).all()), "a token's result is not well formed"
    diff = differing(idx, case.logits64, case.k)
    miss = shortfall(idx, case.logits64, case.k)
    worst = float(miss[diff].max()) / delta if bool(diff.any()) and delta > 0 else 0.0
    print(f"router_pin: E {case.experts} k {case.k} H {case.hidden} T {case.tokens} {case.dtype}: {int(diff.sum())} tokens differ, "
          f"largest shortfall {worst:.3f} delta (delta {delta:.3e})")
    bad = ~excused(idx, gates, case.logits64, case.k, delta)        # a token equal to the fp64 choice must hold its gates too
    assert not bool(bad.any()), f"{int(bad.sum())} unexcused tokens, first {int(bad.nonzero()[0])}"
    assert float(diff.float().mean()) <= DIFFERING_SHARE, f"{int(diff.sum())} of {case.tokens} tokens differ from the fp64 choice"
    return int(diff.sum()), worst


def judge_exact(idx, gates, case):
    """Every slot equals `expected_choice`; the gates match the fp64 softmax of the exact logits within 1e-5 / 1e-4."""
    assert bool(well_formed(idx, gates, case.experts).all()), "a token's result is not well formed"
    want_idx, want_gates = expected_choice(case.logits64, case.k)
    wrong = (idx != want_idx).any(-1)
    if bool(wrong.any()):
        t = int(wrong.nonzero()[0])
        raise AssertionError(f"{int(wrong.sum())} of {case.tokens} tokens differ; token {t}: got {idx[t].tolist()} want {want_idx[t].tolist()} "
                             f"(logits of the wanted {torch.gather(case.logits64[t], 0, want_idx[t].long()).tolist()})")
    torch.testing.assert_close(gates.double(), want_gates, atol=GATE_ATOL, rtol=GATE_RTOL)


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases: (experts, k, hidden, tokens, launch tag)
# ---------------------------------------------------------------------------------------------------------------------------------
DTYPES_16 = (torch.bfloat16, torch.float16)
DTYPES_ALL = (torch.bfloat16, torch.float16, torch.float32)

# MOJO_HIP_GATING=1.  tt rises above 1 only from 512 blocks on (launch_gating); ei = ceil(E / 64) rounded up to the instance
GENERAL_CASES = [
    (64, 8, 72, 2051, "tt4:ei1"),           # 3-of-4 tail in the last block
    (64, 8, 76, 2051, "tt4:ei1"),           # 76 % 8 != 0: the scalar hidden loop for 16-bit types (72 is a multiple of 8)
    (64, 8, 128, 1030, "tt2:ei1"),
    (100, 6, 128, 70, "tt1:ei2"),
    (200, 8, 64, 2051, "tt4:ei4"),
    (320, 8, 136, 1030, "tt2:ei8"),
    (320, 8, 64, 2051, "tt2:ei8"),          # 513 blocks at tt4: the register cap (ei > 4) forces tt2
    (1024, 64, 64, 1030, "tt2:ei16"),
    (5, 5, 64, 16400, "tt4:ei1"),           # sub-wave layout: 8 lanes per token
    (2, 1, 40, 300, "tt1:ei1"),
    (1, 1, 64, 9, "tt1:ei1"),
    (33, 3, 128, 515, "tt1:ei1"),
    # the instances the rows above leave out
    (100, 6, 64, 1030, "tt2:ei2"), (100, 6, 64, 2051, "tt4:ei2"), (200, 8, 64, 70, "tt1:ei4"), (200, 8, 64, 1030, "tt2:ei4"),
    (320, 8, 64, 70, "tt1:ei8"), (1024, 64, 64, 70, "tt1:ei16"),
]

# MOJO_HIP_GATING=2, E = 8
E8_CASES = [
    (8, 1, 512, 33, "e8"), (8, 2, 512, 33, "e8"), (8, 8, 512, 33, "e8"),     # one working wave; a one-token last block
    (8, 2, 1536, 1000, "e8"),                                               # three of four waves working
]

# MOJO_HIP_GATING=3
SMALL_CASES = [
    (64, 8, 4096, 1, "ep64:slices64"),
    (9, 3, 100, 7, "ep16:slices1"),
    (17, 17, 48, 9, "ep32:slices1"),
    (256, 8, 1040, 64, "ep256:slices33"),      # 64 slices wanted, 32 positions each: 33, the last of 16
    (384, 8, 520, 200, "ep256:slices9"),       # two expert chunks; the last slice holds 8 positions of a 16-position step
    (1024, 64, 4104, 256, "ep256:slices4"),    # slice longer than the 512-position LDS image, not a multiple of the step
    (64, 6, 72, 511, "ep64:slices2"),
]

# MOJO_HIP_GATING=4 (16-bit activations, hidden % 64 == 0)
MFMA_CASES = [
    (32, 4, 64, 512, "sk2"),                # sk2 forced to 2 over two K-tiles
    (33, 3, 128, 515, "sk2"),
    (250, 8, 448, 600, "sk2"),              # 7 K-tiles per half; padded columns (e_pad 256)
    (64, 8, 832, 600, "sk4"),               # nkt 13, sk 3 -> sk2 4: 26 tiles over 4 slices (6, 7, 6, 7)
    (64, 8, 1216, 600, "sk4"),              # nkt 19, sk 4: 38 tiles over 4 slices (9, 10, 9, 10)
    (384, 8, 256, 1100, "sk2"),             # two column tiles
    (1024, 64, 64, 520, "sk2"),
]

ROUTES = {"general": ("1", GENERAL_CASES, DTYPES_ALL), "e8": ("2", E8_CASES, DTYPES_16), "small": ("3", SMALL_CASES, DTYPES_ALL),
          "mfma": ("4", MFMA_CASES, DTYPES_16)}


def route_tag(route, suffix):
    return "moe_gating:e8" if route == "e8" else f"moe_gating:{route}:{suffix}"


def exact_case_list():
    """(route, switch value, experts, k, hidden, tokens, tag, dtype, dense) of every exact case."""
    out = []
    for route, (switch, cases, dtypes) in ROUTES.items():
        for experts, k, hidden, tokens, suffix in cases:
            for dtype in dtypes:
                for dense in (True, False):
                    out.append((route, switch, experts, k, hidden, tokens, route_tag(route, suffix), dtype, dense))
    return out


def exact_seed(experts, k, hidden, tokens):
    return (experts * 1000003 + k * 10007 + hidden * 101 + tokens) % (2 ** 31)


# random cases: (experts, k, hidden, tokens, dtype, std, seed, routes), a route being (MOJO_HIP_GATING value or None = by shape,
# launch tag).  The tags follow launch_gating, gate_small_plan and gate_splitk, worked out by hand like the tables above.
def random_case_list():
    out = []
    bf16, fp16, fp32 = torch.bfloat16, torch.float16, torch.float32
    g, s, m = "moe_gating:general:", "moe_gating:small:", "moe_gating:mfma:"
    # the shapes of test_gating_reference_space (tests/test_hip_moe.py): the route each reaches by shape, and the general kernel
    for experts, k, hidden, tokens, by_shape, general in [
            (16, 4, 1024, 64, s + "ep16:slices4", "tt1:ei1"), (32, 8, 1024, 128, s + "ep32:slices8", "tt1:ei1"),
            (64, 8, 1024, 256, s + "ep64:slices16", "tt1:ei1"), (64, 8, 1024, 1024, m + "sk4", "tt2:ei1"),
            (8, 2, 4096, 8192, "moe_gating:e8", "tt2:ei1"), (384, 8, 3584, 128, s + "ep256:slices16", "tt1:ei8"),
            (256, 8, 7168, 77, s + "ep256:slices50", "tt1:ei4"), (5, 5, 200, 33, g + "tt1:ei1", "tt1:ei1"),
            (384, 8, 3584, 2048, m + "sk8", "tt2:ei8"), (256, 8, 7168, 600, m + "sk8", "tt1:ei4"), (33, 3, 128, 515, m + "sk2", "tt1:ei1")]:
        out.append((experts, k, hidden, tokens, bf16, 0.02, 0, ((None, by_shape), ("1", g + general))))
    for dtype in (bf16, fp16):                                               # test_gating_mfma_route_agrees_with_vector_route
        out.append((128, 6, 1024, 768, dtype, 0.05, 3, (("4", m + "sk4"), ("1", g + "tt1:ei2"))))
    for tokens, experts, k, hidden, small, general in [                      # test_gating_few_token_kernel_matches_the_oracle
            (1, 64, 8, 4096, "ep64:slices64", "tt1:ei1"), (7, 9, 3, 100, "ep16:slices1", "tt1:ei1"), (64, 256, 8, 7168, "ep256:slices64", "tt1:ei4"),
            (200, 384, 8, 3584, "ep256:slices10", "tt1:ei8"), (256, 1024, 64, 256, "ep256:slices4", "tt1:ei16"),
            (33, 17, 17, 48, "ep32:slices1", "tt1:ei1"), (64, 64, 6, 4104, "ep64:slices33", "tt1:ei1")]:
        for dtype in (bf16, fp32):
            # (200 tokens: the next seed.  At tokens * 131 + experts the fp32 REFERENCE differs from the fp64 choice on one token of
            # 200, 0.5 %, which the share bound does not allow even to the reference; tests/test_router_pin_golden.py holds every seed to it)
            out.append((experts, k, hidden, tokens, dtype, 0.05, tokens * 131 + experts + (tokens == 200), (("3", s + small), ("1", g + general))))
    for std in (0.0005, 0.002):                                              # fp16 with small weights: w - w_hi inside fp16's subnormals
        out.append((64, 8, 1024, 8192, fp16, std, 7, (("1", g + "tt4:ei1"), ("4", m + "sk4"))))
        out.append((64, 8, 1024, 256, fp16, std, 7, (("3", s + "ep64:slices16"),)))
    return out
