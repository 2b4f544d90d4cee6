"""Which K positions does the sampling selection choose, and in which order?  The host side of DESIGN §4.24 (numpy and
plain torch, no GPU).

`csrc/sampling.hip` selects with a six-pass radix select over the composites ``key << 32 | ~index`` (key digits of 12 + 10 + 10
bits, then the same three digits of ``~index``), once per segment in pass A and once per row in pass B, and leaves the search
as soon as the chosen bin holds exactly what is still needed.  The rule "among equal values the lower index first, a tie across
position K keeps the lower indices" lives in the last three passes and in the ``c >= threshold`` compaction.  This module holds

* `expected_topk`: that rule written independently of the golden (``numpy.lexsort``; `oracle.sampling.topk_sorted`, a stable
  torch sort, stays the golden and tests/test_sampling_pin_golden.py holds the two equal on every case);
* `geometry`: a mirror of ``make_geometry`` / ``segment_range``, used only to PLACE values and to ACCOUNT for what a case
  reaches, never to produce an expected output; it is checked against ``mojo_hip_sampling_workspace_bytes`` on the host and
  against the ``slices{S}x{sub}`` suffix of the launch tag on the device;
* `search_depth`: a model of ``select_threshold``'s digit walk, for the accounting only (`cut_depth` is its closed form);
* the case builders: deterministic rows built from bit patterns, so that "adjacent representable values" is exact in fp32,
  bf16 and fp16.  Each returns ``(logits, k, note)``; `CASES` names them and `get_case` adds ``top_p``.

Which search depth a dtype can reach (`REACHABLE`): the fp32 image of a bf16 / fp16 value has 16 / 13 zero low bits, so the
third key digit (bits 9..0) is the same for every key under one prefix and can never be the pass that ends the search: depth 3
is fp32 only.  Depth 4, the first index digit (``~index`` bits 31..20), separates nothing below 2^20 columns; only the
`first_index_digit` family is that wide, and it is built in bf16 and fp32 (4 MB a row), so no fp16 row reaches depth 4.
"""
import functools
from types import SimpleNamespace

import numpy as np
import torch

NEG_INF = -float("inf")
FP32, BF16, FP16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = (FP32, BF16, FP16)
SHORT = {FP32: "fp32", BF16: "bf16", FP16: "fp16"}
SLICES = (0, 1, 2, 3, 8, 4096)           # every case runs with each of these on the device
MAX_K, SEG_KEYS, CUS, MAX_SLICES = 1024, 16384, 256, 4096      # kMaxK, kSegKeys, kCUs and the cap of make_geometry
DIGITS = (12, 10, 10, 12, 10, 10)        # key bits 31..20, 19..10, 9..0, then the same of ~index
REACHABLE = {FP32: {0, 1, 2, 3, 4, 5, 6}, BF16: {0, 1, 2, 4, 5, 6}, FP16: {0, 1, 2, 5, 6}}    # module docstring
ONE = {FP32: 0x3F800000, BF16: 0x3F80, FP16: 0x3C00}            # the bit pattern of 1.0


# ---------------------------------------------------------------------------------------------------------------------------------
# the rule
# ---------------------------------------------------------------------------------------------------------------------------------
def expected_topk(logits32, k):
    """(values fp32 [rows, k], indices int64 [rows, k]): positions sorted by (value descending, index ascending), -0.0 equal
    to +0.0, the first k of them."""
    x = logits32.reshape(-1, logits32.shape[-1])
    vals, idxs = [], []
    for row in x.double().numpy():
        row = row + 0.0                                              # -0.0 + 0.0 == +0.0: one zero
        order = np.lexsort((np.arange(row.size), -row))[:k]          # last key first: -value, then index
        idxs.append(order)
        vals.append(row[order])
    return torch.from_numpy(np.stack(vals)).float(), torch.from_numpy(np.stack(idxs)).long()


# ---------------------------------------------------------------------------------------------------------------------------------
# the mirror of make_geometry / segment_range
# ---------------------------------------------------------------------------------------------------------------------------------
def _ceil_div(a, b):
    return -(-a // b)


def _round_up(a, b):
    return _ceil_div(a, b) * b


@functools.lru_cache(maxsize=None)
def geometry(rows, vocab, k, slices):
    """slices, sub, seg_len, kcap, the [start, end) of every segment, the launch tag's suffix and the workspace bytes."""
    k = min(k, vocab)
    s = slices
    if s <= 0:
        s = _ceil_div(CUS, max(rows, 1))
        s = min(s, max(vocab // (4 * k), 1))
        s = max(s, _ceil_div(vocab, SEG_KEYS))
    s = min(s, _ceil_div(vocab, 64), MAX_SLICES)
    slice_len = _round_up(_ceil_div(vocab, s), 64)
    s = _ceil_div(vocab, slice_len)
    sub = _ceil_div(slice_len, SEG_KEYS)
    seg_len = _round_up(_ceil_div(slice_len, sub), 64)
    segments = []
    for seg in range(s * sub):
        sl, j = divmod(seg, sub)
        s1 = min(sl * slice_len + slice_len, vocab)
        start = sl * slice_len + j * seg_len
        segments.append((start, max(min(start + seg_len, s1), start)))
    kcap = min(k, seg_len)
    return SimpleNamespace(slices=s, sub=sub, slice_len=slice_len, seg_len=seg_len, nseg=s * sub, kcap=kcap, segments=tuple(segments),
                           tag=f"slices{s}x{sub}", bytes=rows * s * sub * kcap * 8)


def boundaries(rows, vocab, k, which=SLICES):
    """The interior segment boundaries of the geometries `which`, sorted."""
    out = set()
    for s in which:
        out.update(e for _, e in geometry(rows, vocab, k, s).segments if 0 < e < vocab)
    return sorted(out)


# ---------------------------------------------------------------------------------------------------------------------------------
# the model of select_threshold
# ---------------------------------------------------------------------------------------------------------------------------------
def composites_of(row):
    """uint64 ``key << 32 | ~index`` of one row (any of the three dtypes), as key_of / composite build them."""
    u = row.float().numpy().view(np.uint32).copy()
    u[u == 0x80000000] = 0
    key = np.where(u & 0x80000000, ~u, u | np.uint32(0x80000000)).astype(np.uint64)
    return (key << np.uint64(32)) | (~np.arange(u.size, dtype=np.uint32)).astype(np.uint64)


def search_walk(composites, need):
    """The (digit, count in the chosen bin, still needed) of every pass that select_threshold runs; [] for need >= n."""
    live = [int(c) for c in composites]
    if need >= len(live):
        return []
    out, shift = [], 64
    for width in DIGITS:
        shift -= width
        hist = {}
        for c in live:
            d = (c >> shift) & ((1 << width) - 1)
            hist[d] = hist.get(d, 0) + 1
        above = 0
        for d in sorted(hist, reverse=True):
            if need <= above + hist[d]:
                break
            above += hist[d]
        need -= above
        out.append((d, hist[d], need))
        live = [c for c in live if (c >> shift) & ((1 << width) - 1) == d]
        if hist[d] == need:
            break
    return out


def search_depth(composites, need):
    """The pass (1..6) at which the search ends; 0 for need >= n."""
    return len(search_walk(composites, need))


def cut_depth(composites, need):
    """`search_depth` in closed form: the bins are contiguous in sorted order, so the chosen bin holds exactly what is needed
    as soon as the first excluded composite leaves the prefix of the last taken one: the digit of their highest differing bit."""
    c = np.asarray(composites, dtype=np.uint64)
    if need >= c.size:
        return 0
    part = np.partition(c, c.size - need - 1)
    high = (int(part[c.size - need:].min()) ^ int(part[c.size - need - 1])).bit_length() - 1
    edge = 64
    for depth, width in enumerate(DIGITS, 1):
        edge -= width
        if high >= edge:
            return depth
    raise AssertionError("two equal composites")


def candidates_of(comps, geo, k):
    """Per segment the composites pass A writes (its top min(k, length)), for one row."""
    out = []
    for start, end in geo.segments:
        seg = comps[start:end]
        take = min(k, seg.size)
        out.append(np.sort(seg)[seg.size - take:])
    return out


def depths(row, geo, k, walk=cut_depth):
    """(the depth of every non-empty segment's search in pass A, the depth of pass B) for one row under one geometry."""
    comps = composites_of(row)
    a = [walk(comps[s:e], min(k, e - s)) for s, e in geo.segments if e > s]
    return a, walk(np.concatenate(candidates_of(comps, geo, k)), k)


# ---------------------------------------------------------------------------------------------------------------------------------
# values from bit patterns
# ---------------------------------------------------------------------------------------------------------------------------------
def from_ordinals(ordinals, dtype):
    """The value whose sign-magnitude bit pattern is the ordinal: n > 0 is the n-th positive value above +0.0, n < 0 the
    |n|-th below it, so consecutive ordinals are adjacent representable values of `dtype`."""
    o = np.asarray(ordinals, dtype=np.int64)
    sign = 1 << (31 if dtype == FP32 else 15)
    bits = np.where(o >= 0, o, -o | sign)
    if dtype == FP32:
        return torch.from_numpy(bits.astype(np.uint32).view(np.float32).copy())
    return torch.from_numpy(bits.astype(np.uint16).view(np.int16).copy()).view(dtype)


def scatter(n, vocab):
    """n distinct positions, a fixed permutation of the columns (7919 is prime and divides no vocabulary used here)."""
    assert vocab % 7919 != 0 and n <= vocab
    return (np.arange(n, dtype=np.int64) * 7919 + 13) % vocab


def _levels(vocab, dtype, levels=50, base=None):
    """A heavily quantised row: `levels` adjacent values from 1.0 up, each about vocab / levels times, columns permuted."""
    base = ONE[dtype] if base is None else base
    return from_ordinals(base + scatter(vocab, vocab) % min(levels, vocab), dtype)


def _note(family, text, claims=(), **kw):
    return dict(family=family, text=text, claims=list(claims), keep=kw.pop("keep", 1), filter_value=kw.pop("filter_value", NEG_INF),
                sample=kw.pop("sample", False), **kw)


# ---------------------------------------------------------------------------------------------------------------------------------
# the families.  A claim is (slices, kind, row, value): "a" some segment of pass A ends at depth value, "b" pass B does,
# "a_bin4" / "b_bin4" the digit chosen in the fourth pass, "straddle" the tie group at the cut crosses position K,
# "span" that group has members in at least `value` segments.
# ---------------------------------------------------------------------------------------------------------------------------------
def constant(dtype, k, vocab=40000):
    x = torch.empty(3, vocab, dtype=dtype)
    x[0] = from_ordinals([ONE[dtype] + 3], dtype)
    x[1] = from_ordinals([-(ONE[dtype] + 3)], dtype)
    x[2] = 0.0
    x[2, ::2] = -0.0                                                 # both zeros: one value
    claims = [(s, "straddle", r, True) for s in (0, 1) for r in range(3)]
    claims += [(1, "span", r, 3) for r in range(3)] + [(0, "span", r, geometry(3, vocab, k, 0).nseg) for r in range(3)]
    claims += [(1, "a", 0, 6), (1, "b", 0, 5)]    # pass B: the first segment's K lowest columns are all of the first block's
    return x, k, _note("constant", "a positive, a negative and a +-0.0 constant row: indices 0..K-1", claims, sample=True)


def _cut_at_block_edge(positions, wanted):
    """The count n nearest to `wanted` such that the n-th and (n+1)-th of the sorted positions lie in different 1024-blocks."""
    p = np.sort(np.asarray(positions))
    edges = np.nonzero(p[1:] // 1024 != p[:-1] // 1024)[0] + 1
    return int(edges[np.abs(edges - wanted).argmin()])


def two_level(dtype, k, vocab=40000):
    """Rows (i), (ii), (iii): `a` above `b` above a constant background, count(a) < K < count(a) + count(b).  `b` sits at the
    first and last key and on both sides of every segment boundary: of slices 1, 2, 3 and 8 in rows (i) and (ii), whose count
    of `b` is held near K, and of all six slice counts (625 boundaries 64 columns apart among them) in row (iii)."""
    rows = 3
    a, b, back = (from_ordinals([ONE[dtype] + n], dtype) for n in (40, 20, -ONE[dtype]))
    few = boundaries(rows, vocab, k, (1, 2, 3, 8))
    edge = lambda cuts: [0, vocab - 1] + [p for c in cuts for p in (c - 1, c)]           # noqa: E731
    x = torch.empty(rows, vocab, dtype=dtype)
    x[:] = back
    count_a = []
    # (i) the needed b all in the first aligned 1024-index block, more of them there than needed: index digit 3
    pos_b = sorted(set(edge(few) + list(range(0, 1024, 3 if k >= 256 else 11))))
    in_block = sum(p < 1024 for p in pos_b)
    count_a.append(k - in_block * 2 // 3)
    # (ii) the b more than a block apart, the cut between two blocks: index digit 2
    pos_b2 = sorted(set(edge(few) + list(range(1500, vocab, 1500 if k < 256 else 97))))
    count_a.append(k - _cut_at_block_edge(pos_b2, k // 3))
    # (iii) thousands of b: every segment's own top kcap is one tie, pass B sees about nseg x kcap equal keys
    pos_b3 = sorted(set(edge(boundaries(rows, vocab, k)) + list(range(5, vocab, 7))))
    count_a.append(k // 8)
    for r, pos in enumerate((pos_b, pos_b2, pos_b3)):
        taken = set(pos)
        where_a = [p for p in scatter(vocab, vocab) if p not in taken][: count_a[r]]
        assert len(where_a) == count_a[r] and 0 < count_a[r] < k < count_a[r] + len(pos)
        x[r, pos] = b
        x[r, where_a] = a
    claims = [(s, "straddle", r, True) for s in (0, 1) for r in range(rows)]
    claims += [(0, "b", 0, 6), (1, "a", 0, 6), (0, "b", 1, 5), (1, "b", 1, 5), (1, "span", 1, 3),
               (0, "span", 2, geometry(rows, vocab, k, 0).nseg), (4096, "span", 2, geometry(rows, vocab, k, 4096).nseg)]
    return x, k, _note("two_level", "(i) cut inside one 1024-block, (ii) cut between blocks, (iii) thousands tied", claims, sample=True)


def two_level_wide(dtype=BF16, k=1000, vocab=151936):
    """Row (iii) at the vocabulary of the flagship shapes, one row."""
    a, b, back = (from_ordinals([ONE[dtype] + n], dtype) for n in (40, 20, -ONE[dtype]))
    x = torch.empty(1, vocab, dtype=dtype)
    x[:] = back
    cuts = boundaries(1, vocab, k)
    pos = sorted(set([0, vocab - 1] + [p for c in cuts for p in (c - 1, c)] + list(range(5, vocab, 7))))
    taken = set(pos)
    where_a = [p for p in scatter(4 * k, vocab) if p not in taken][: k // 8]
    x[0, pos] = b
    x[0, where_a] = a
    claims = [(0, "straddle", 0, True), (0, "span", 0, geometry(1, vocab, k, 0).nseg), (1, "span", 0, geometry(1, vocab, k, 1).nseg)]
    return x, k, _note("two_level", "(iii) on 151 936 columns", claims, sample=True)


@functools.lru_cache(maxsize=None)
def straddling_vocab(k=300, rows=1, margin=1536):
    """The first V above 2^20 (a multiple of 64) at which the segment that holds column 2^20 reaches `margin` columns to
    both sides of it under slices=0 and slices=1 (K 300, one row: 1 049 216 is the first at a margin of 64)."""
    for vocab in range((1 << 20) + 64, (1 << 20) + (1 << 16), 64):
        ok = True
        for s in (0, 1):
            start, end = next((a, b) for a, b in geometry(rows, vocab, k, s).segments if a <= (1 << 20) < b)
            ok &= (1 << 20) - start >= margin and end - (1 << 20) >= margin
        if ok:
            return vocab
    raise AssertionError("no such vocabulary")


def _straddle_row(dtype, vocab, k, below, above):
    """100 `a`, then a tie group with `below` members under column 2^20, `above` from it on inside the straddling segment
    (every second / third column), and 52 more far behind it in other segments; a constant background under both."""
    a, t, back = (from_ordinals([ONE[dtype] + n], dtype) for n in (40, 20, -ONE[dtype]))
    m = 1 << 20
    x = torch.empty(vocab, dtype=dtype)
    x[:] = back
    x[m - 1500: m - 1400] = a
    x[[m - 1 - 2 * j for j in range(below)]] = t
    x[[m + 3 * j for j in range(above)]] = t
    x[[m + 20000 + 7 * j for j in range(50)] + [vocab - 1, vocab - 5000]] = t
    return x


def first_index_digit(dtype, variant):
    """K 300 = 100 `a` + 200 of the tie group.  'second': 120 members below 2^20, fewer than the 200 needed: the fourth pass
    chooses the SECOND bin (0xFFE) of ~index bits 31..20.  'exact': exactly 200 below: the search ends in the fourth pass."""
    k = 300
    rows = {"second": [(120, 150)], "exact": [(200, 150)], "both": [(120, 150), (200, 150)]}[variant]
    vocab = straddling_vocab(k, len(rows))
    x = torch.stack([_straddle_row(dtype, vocab, k, lo, hi) for lo, hi in rows])
    claims = []
    for r, (lo, _) in enumerate(rows):
        for s in (0, 1):
            claims += [(s, "straddle", r, True)]
            claims += [(s, "a_bin4", r, 0xFFE if lo < 200 else 0xFFF), (s, "b_bin4", r, 0xFFE if lo < 200 else 0xFFF)]
            if lo == 200:
                claims += [(s, "a", r, 4), (s, "b", r, 4)]
    return x, k, _note("first_index_digit", f"a tie group across column 2^20 ({variant})", claims)


# the step, in ordinals of the dtype, that changes the key first in digit 1, 2, 3 (None: the dtype has no such step), and the
# lowest of the K + margin top ordinals: 16 bf16 values share one first digit, so its digit-2 rows cut inside such a group
_STEP = {FP32: {1: 1 << 20, 2: 1 << 10, 3: 1}, BF16: {1: 16, 2: 1}, FP16: {1: 128, 2: 1}}
_LOW = {FP32: {1: 0x3D800000, 2: ONE[FP32], 3: ONE[FP32]}, BF16: {1: 0x3D80, 2: ONE[BF16]}, FP16: {1: 0x2C00, 2: ONE[FP16]}}
_SMALL = {FP32: 0x3B800000, BF16: 0x3B80, FP16: 0x1C00}          # 2^-8, under every positive top value
_LARGE = {FP32: 0x42800000, BF16: 0x4280, FP16: 0x5400}          # 64, above every top magnitude


def key_digits(dtype, digit, repeat, vocab=16000, k=64, margin=8):
    """No ties (repeat 1): the top K + margin values are `step` ordinals apart, scattered by a fixed permutation over a lower
    background; a positive row, a negative row (the ~u branch of key_of) and one of subnormals around zero.  repeat 3: every
    value three times, so the cut falls inside a triple and needs key AND index digits."""
    n = k + margin
    step, low = _STEP[dtype][digit], _LOW[dtype][digit]
    x = torch.empty(3, vocab, dtype=dtype)
    where = scatter(n * repeat, vocab)
    which = np.arange(n * repeat) // repeat
    x[0] = from_ordinals([_SMALL[dtype]], dtype)
    x[0, where] = from_ordinals(low + which * step, dtype)
    x[1] = from_ordinals([-_LARGE[dtype]], dtype)
    x[1, where] = from_ordinals(-(low + (which + 8) * step), dtype)
    x[2] = from_ordinals([-ONE[dtype]], dtype)
    x[2, where] = from_ordinals(which - n // 2, dtype)               # ordinals -36 .. 35: subnormals, +0.0, no -0.0
    claims = []
    for r in (0, 1):
        if repeat == 1:                                              # slices=1 is one segment: pass A is the whole search
            claims += [(1, "a", r, digit), (1, "b", r, 0), (0, "b", r, digit), (0, "straddle", r, False)]
        else:
            claims += [(0, "straddle", r, True), (1, "straddle", r, True)]
    claims += [(0, "straddle", 2, repeat == 3)]
    return x, k, _note("key_digits", f"top values differ first in key digit {digit}, each {repeat} x", claims)


def minus_inf(dtype, filter_value, vocab=40000, k=64):
    """Fewer finite logits than K, in the last 64 columns (the last segment of every geometry) or the first 64 only; and a row
    with exactly K finite ones."""
    x = torch.full((3, vocab), NEG_INF, dtype=dtype)
    x[0, [vocab - 64 + 2 * j for j in range(30)]] = from_ordinals(ONE[dtype] + np.arange(30), dtype)
    x[1, [2 * j + 1 for j in range(30)]] = from_ordinals(ONE[dtype] + np.arange(30)[::-1].copy(), dtype)
    x[2, scatter(k, vocab)] = from_ordinals(ONE[dtype] + np.arange(k), dtype)
    claims = [(s, "straddle", r, True) for s in (0, 1) for r in (0, 1)] + [(0, "straddle", 2, False)]
    return x, k, _note("minus_inf", "the cut lies among the -inf keys; exactly K finite", claims, filter_value=filter_value, sample=True)


def edge_k(dtype, k, vocab=40000, rows=2, keep=1):
    x = torch.stack([_levels(vocab, dtype, 50), _levels(vocab, dtype, 7, ONE[dtype] - 3)][:rows])
    claims = [(0, "straddle", 0, True)] if k < vocab and vocab >= 40000 else []      # 800 columns a level: a tie across K
    return x, k, _note("edges", f"K {k} of {vocab} quantised columns, min_tokens_to_keep {keep}", claims, keep=keep)


CASES = {}


def _add(name, fn, *args, dtypes=DTYPES):
    for dtype in dtypes:
        CASES[f"{name}-{SHORT[dtype]}"] = (fn, (dtype,) + args)


_add("constant-k64", constant, 64)
_add("constant-k1024", constant, 1024)
_add("two_level-k64", two_level, 64)
_add("two_level-k1024", two_level, 1024)
_add("two_level-wide", two_level_wide, dtypes=(BF16,))
_add("first_index_digit-both", first_index_digit, "both", dtypes=(BF16,))
_add("first_index_digit-second", first_index_digit, "second", dtypes=(FP32,))
_add("first_index_digit-exact", first_index_digit, "exact", dtypes=(FP32,))
for _digit in (1, 2, 3):
    for _repeat in (1, 3):
        _add(f"key_digits-d{_digit}x{_repeat}", key_digits, _digit, _repeat, dtypes=[d for d in DTYPES if _digit in _STEP[d]])
_add("minus_inf", minus_inf, NEG_INF)
_add("minus_inf-finite_filter", minus_inf, -4.0)
for _k in (1, 2, 3, 1023, 1024):
    _add(f"edges-k{_k}", edge_k, _k)
for _v in (1, 63, 64, 65, 1024):
    _add(f"edges-k_is_v{_v}", edge_k, _v, _v, 1)
_add("edges-v65-k3", edge_k, 3, 65)
_add("edges-odd_vocab", edge_k, 300, 50001)                      # rows not 16-byte aligned: scalar staging, a short last segment
_add("edges-keep_above_cut", edge_k, 64, 40000, 2, 60)
_add("edges-keep_is_k", edge_k, 64, 40000, 2, 64)
MISALIGNED = ("two_level-k64", "constant-k1024", "edges-k1023")   # V % 8 == 0: only the base pointer takes the narrow loop


def choose_top_p(values32):
    """The first of 0.7005, 0.7010, ... that the fp64 running sum of the sorted values stays 4 delta away from on every row,
    delta = 8 x the fp32 running sum's own deviation (tests/sampling_judge.py): no row undecidable, by construction."""
    cum32 = values32.softmax(-1).cumsum(-1)
    cum64 = torch.softmax(values32.double(), -1).cumsum(-1)
    delta = 8 * float((cum32.double() - cum64).abs().max())
    for j in range(1, 200):
        top_p = round(0.7 + 0.0005 * j, 4)
        if float((cum64 - float(torch.tensor(top_p, dtype=torch.float32))).abs().min()) > 4 * delta + 1e-12:
            return top_p
    raise AssertionError("no decidable top_p")


@functools.lru_cache(maxsize=None)
def get_case(name):
    fn, args = CASES[name]
    logits, k, note = fn(*args)
    assert logits.dim() == 2 and 1 <= logits.shape[0] <= 4 and k <= MAX_K and logits.dtype == args[0]
    values, indices = expected_topk(logits.float(), k)
    return SimpleNamespace(name=name, logits=logits, k=k, dtype=logits.dtype, rows=logits.shape[0], vocab=logits.shape[1],
                           top_p=choose_top_p(values), keep=note["keep"], filter_value=note["filter_value"], note=note,
                           family=note["family"], values=values, indices=indices)


@functools.lru_cache(maxsize=None)
def judged_of(name):
    from sampling_judge import Judged

    c = get_case(name)
    return Judged(c.logits, c.top_p, c.keep, c.k, c.filter_value)


def judge_filter(name, probs, indices, what):
    """What the device test asserts on one filter result (and what the host test feeds wrong answers to)."""
    c, judged = get_case(name), judged_of(name)
    indices = indices.reshape(c.rows, c.k).cpu()
    assert indices.dtype == torch.int64
    assert torch.equal(indices, judged.indices) and torch.equal(indices, c.indices), f"{what}: indices differ from the golden's"
    judged.check(probs, indices, c.dtype, what, cap=0.0)
    if c.filter_value == NEG_INF:
        removed = torch.arange(c.k).expand(c.rows, c.k) >= judged.kept.unsqueeze(-1)
        assert not probs.reshape(c.rows, c.k).cpu()[removed].any(), f"{what}: a probability past the cut is not 0"
