"""The NSA pin: inputs that make the output of `MojoDecodeNSA` / `MojoPrefillNSA` (and their paged forms) a
read-out of the keys a (row, head) attends, the expectation and the comparer.

V is one-hot per key (``V[t] = 8 e_(t mod P)``), so channel ``c`` reads ``8 sum w_t`` over ``t = c (mod P)``; the gate is driven
to 0 / 1 per branch (four legs); all keys of a (sequence, head) are equal (uniform softmaxes, tied block scores: the "equal"
family).  The expectation is always the fp64 model of
tests/nsa_golden.py / tests/nsa_prefill_golden.py on the stored inputs; `weights_one` hands out the same model's per-key weights
(and, on request, a deliberately WRONG model's) for the sensitivity condition, the comparer's key lists and the CPU tests."""
import functools
import math

import numpy as np
import torch

import nsa_golden as G
import nsa_prefill_golden as GP

HEADS, AMP = 2, 8.0
UNIT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
BF16, FP16 = torch.bfloat16, torch.float16
NAMES = ("compress_ratio", "block_size", "num_selected_blocks", "window_size")
LEGS = {"compressed": (1, -1, -1), "selected": (-1, 1, -1), "window": (-1, -1, 1), "all": (0, 0, 0)}   # the sign of q . gate_j
BRANCH = {"compressed": 0, "selected": 1, "window": 2}
# "equal" reads the compressed range, the window and the tie rule; "graded" reads which blocks the selection takes (its other
# softmaxes are peaked on the best block, so the compressed-alone and window-alone legs would not be pins)
FAMILY_LEGS = {"equal": ("compressed", "selected", "window", "all"), "graded": ("selected", "all")}
MAX_KEYS = 1100

# (cr, bs, nsel, ws), head_dim, dtype, page of the paged run
DECODE = (((1, 16, 3, 16), 64, BF16, 16), ((2, 2, 64, 0), 128, FP16, 48), ((3, 48, 2, 50), 64, FP16, 16),
          ((5, 40, 1, 7), 128, BF16, 128), ((4, 8, 3, 20), 64, BF16, 256), ((16, 16, 5, 100), 128, FP16, 48),
          ((32, 64, 2, 33), 64, FP16, 128), ((4, 32, 0, 48), 128, BF16, 16), ((4, 64, 16, 512), 64, BF16, 256))
DECODE_HOLE = ((3, 48, 2, 50), 5)        # pages of 16: key 80 is neither a block (48) nor a group (3) edge
# ..., page, table width (None: two columns more than needed), is_causal values, the tag's waves
PREFILL = (((1, 16, 2, 5), 64, BF16, 16, None, (True,), 4), ((2, 6, 3, 16), 128, FP16, 48, None, (True,), 4),
           ((4, 32, 2, 48), 64, BF16, 128, None, (True, False), 4), ((8, 24, 2, 17), 128, BF16, 16, None, (True,), 4),
           ((16, 16, 3, 40), 64, FP16, 256, None, (True, False), 4), ((16, 64, 0, 0), 128, FP16, 48, None, (True,), 4),
           ((2, 4, 4, 9), 64, BF16, 16, 62, (True,), 2), ((2, 2, 3, 9), 128, BF16, 128, 8, (True,), 1))
PREFILL_HOLE = ((8, 24, 2, 17), 1)       # pages of 16: key 16 is no block edge (24); a page edge is always a group edge (cr | 16)
SPLITS = (1, 2, 5, "tiles", None)


def cfg_of(t):
    return dict(zip(NAMES, t))


def lengths(cr, bs, nsel, ws, page=None, most=MAX_KEYS):
    """The lengths of a configuration: both sides of every edge the kernels compute with, and one ragged length near 1000."""
    ragged = next(n for n in range(997, 1100) if n % 16 and n % bs and (cr == 1 or n % cr))
    pages = [] if page is None else [page - 1, page, page + 1]
    want = [0, 1, cr - 1, cr, cr + 1, bs - 1, bs, bs + 1, ws - 1, ws, ws + 1, nsel * bs, nsel * bs + 1] + pages + [255, 256, 257, ragged]
    return tuple(sorted({n for n in want if 0 <= n <= most}))


def graded_most(t):
    """The longest row of the graded family.  Its taken blocks weigh 1, e^-step, e^-2 step, ...; a key of the k-th weighs about
    ``e^(-(k - 1) step) / bs`` and is seen (``8 w >= 2 bound``, bound >= 2^-9) down to about 2^-10.5.  Where ``nsel`` blocks
    cannot all be seen, rows are cut to as many blocks as can (``nsel >= nb`` on every row then)."""
    cr, bs, nsel, _ = t
    step = 1.5                                                          # the smallest the builder tries: e^1.5 > 4
    seen = 1 + int((10.5 * math.log(2) - math.log(bs)) // step)
    return MAX_KEYS if nsel <= seen else seen * bs


def decode_lens(t, page, most=None):
    return lengths(*t, page, most or (MAX_KEYS if t != (4, 64, 16, 512) else 512))   # the defaults: nsel >= nb and ws >= sl on every row


def prefill_seqs(t, page, many=None, most=MAX_KEYS):
    """(q_len, kv_len) pairs: a sequence of at least 66 rows crossing cr, bs and ws; an empty one; rows straddling a block (and
    group) edge over a long cache; one row over many keys; q_len > kv_len — the last three on the paged op only."""
    cr, bs, nsel, ws = t
    if most < 66:                                 # a cut graded case: every prefix of the longest row, and q_len > kv_len
        short = ((most, most), (0, 0), (min(cr + 1, most), min(cr + 1, most)))
        return short if page is None else short + ((most + 3, most),)
    full = min(max(66, min(max(cr, bs, ws) + 2, 80)), most)
    if page is None:
        return ((full, full), (0, 0), (cr + 1, cr + 1), (3, 3))
    edge = min(max(2, 150 // bs) * bs, most - bs) + 2
    many = min(many or 300 + cr + 1, most - 1)
    return ((full, full), (0, 0), (5, edge), (1, many), (12, 7), (cr + 1, 2 * bs + cr))


def weights_one(q, k, gate, scale, compress_ratio, block_size, num_selected_blocks, window_size, wrong=None, scores_out=None):
    """`nsa_golden.model_one`'s weights: q [H,D], k [sl,H,D], gate [H,D,3] in fp64 -> (w [3,H,sl], taken blocks per head), with
    ``out = sum_t (w[0] + w[1] + w[2])[:, t, None] v[t]``.  ``wrong`` names ONE deliberate mistake (the CPU tests' wrong models)."""
    sl, heads, _ = k.shape
    cr, bs, nsel, ws = compress_ratio, block_size, num_selected_blocks, window_size
    ws = max(0, ws + {"ws+1": 1, "ws-1": -1}.get(wrong, 0))
    n_groups, nb, gpb = (-(-sl // cr) if wrong == "ceil groups" else sl // cr), -(-sl // bs), bs // cr
    w, taken = np.zeros((3, heads, sl)), []
    for h in range(heads):
        s = scale * k[:, h] @ q[h]
        g = 1.0 / (1.0 + np.exp(-(q[h] @ gate[h])))
        scores = np.zeros(nb)
        if n_groups:
            starts = np.arange(0, n_groups * cr, cr)
            size = np.minimum(starts + cr, sl) - starts
            pc = G._softmax(np.add.reduceat(s[:min(n_groups * cr, sl)], starts) / size)
            w[0, h, :min(n_groups * cr, sl)] = np.repeat(g[0] * pc / size, size)
            part = np.add.reduceat(pc, np.arange(0, n_groups, gpb))
            scores[:part.size] = part
        n_taken = max(0, min(nsel, nb) - (wrong == "one block fewer"))
        chosen = sorted(range(nb), key=lambda b: (-scores[b], -b if wrong == "tie high" else b))[:n_taken]
        taken.append(chosen)
        if scores_out is not None:
            scores_out.append(scores)
        end = {"block short": -1, "block long": 1}.get(wrong, 0)
        keys = [np.arange(b * bs, max(b * bs, min(min((b + 1) * bs, sl) + end, sl))) for b in sorted(chosen)]
        keys = np.unique(np.concatenate(keys)) if keys else np.arange(0)
        w[1, h, keys] = g[1] * G._softmax(s[keys])
        win = np.arange(max(0, sl - ws), sl)
        w[2, h, win] = g[2] * G._softmax(s[win])
    return w, taken


def rows_of(c):
    """(output row, sequence, row of the sequence, keys seen, kv_len) of every output row of a case."""
    if c["op"] == "decode":
        return [(i, i, 0, sl, sl) for i, sl in enumerate(c["lens"].tolist())]
    out, row = [], 0
    for i, (q_len, kv_len) in enumerate(c["seqs"]):
        for t in range(q_len):
            out.append((row, i, t, min(max(kv_len - q_len + t + 1 if c["causal"] else kv_len, 0), kv_len), kv_len))
            row += 1
    return out


def row_weights(c, row, seq, t_kv, wrong=None, key=None, scores_out=None):
    """The weights [3,H,t_kv'] of one output row (prefill: the ``0 < t_kv < cr`` rule of `nsa_prefill_golden.model`)."""
    key, cfg = c["key"] if key is None else key, c["cfg"]
    if c["op"] == "prefill":
        t_kv = min(max(t_kv + {"t_kv+1": 1, "t_kv-1": -1}.get(wrong, 0), 0), c["seqs"][seq][1])
        if 0 < t_kv < cfg["compress_ratio"] and wrong != "short rows as decode":
            cfg = dict(cfg, compress_ratio=1, block_size=max(cfg["block_size"], t_kv))
    return weights_one(c["query"][row].double().numpy(), key[seq, :t_kv].double().numpy(), c["gate"].double().numpy(), c["scale"],
                       **cfg, wrong=wrong, scores_out=scores_out)


def out_of_weights(c, wrong=None, key=None, value=None):
    """``out64`` rebuilt from the per-key weights (of the true model, or of a wrong one)."""
    value = c["value"] if value is None else value
    out = np.zeros(tuple(c["query"].shape))
    for row, seq, _, t_kv, _ in rows_of(c):
        w = row_weights(c, row, seq, t_kv, wrong, key)[0].sum(axis=0)
        out[row] = np.einsum("ht,thd->hd", w, value[seq, :w.shape[1]].double().numpy())
    return torch.from_numpy(out)


def _dyadic(x):
    """Multiples of 1/16 in [-3, 3]: every product and every partial sum of a score is exact in fp32 and fp64 in any order, so
    equal keys give bit-equal scores — in the fp64 model too, whose matrix products do not promise one order per row."""
    return (x * 16).round().clamp(-48, 48) / 16


def _inputs(op, t, dim, dtype, sizes, seed):
    """The query (one per head, on every row) and the keys (one per (sequence, head), on every key) of a geometry."""
    cr, bs, nsel, ws = t
    gen, scale = torch.Generator().manual_seed(seed), 0.125      # a power of two for both head sizes: scaled scores stay exact
    qh = _dyadic(torch.randn(HEADS, dim, generator=gen)).to(dtype)
    qq = (qh.double() ** 2).sum(-1)
    kv = [s if op == "decode" else s[1] for s in sizes]
    cap = max(max(kv), 1)
    key = torch.full((len(kv), cap, HEADS, dim), float("nan"), dtype=torch.float64)
    for i, sl in enumerate(kv):
        for h in range(HEADS):
            key[i, :sl, h] = _dyadic(torch.randn(dim, generator=gen)).double()
    rows = len(kv) if op == "decode" else sum(s[0] for s in sizes)
    return qh[None].expand(rows, HEADS, dim).contiguous(), key.to(dtype), qh, qq, scale, kv


def _value(kv, period, dim, dtype):
    cap = max(max(kv), 1)
    v = torch.full((len(kv), cap, HEADS, dim), float("nan"), dtype=dtype)
    for i, sl in enumerate(kv):
        v[i, :sl] = (AMP * torch.eye(dim)[torch.arange(sl) % period])[:, None, :].to(dtype)
    return v


def graded_levels(kv, bs, nsel, seed):
    """Per (sequence, head) a seeded permutation of ``0 .. nb - 1`` in which the taken blocks of EVERY prefix have adjacent
    levels (a taken block ``k`` levels below the best weighs ``e^(-k step)`` and could not be seen otherwise): a seeded half of
    the blocks (on head 1 all of them), the first ``nsel`` and the last one always, are "climbers" whose levels rise with the index above
    all others; the rest take a seeded permutation of the low levels.  Every prefix then takes its last ``nsel`` climbers: late
    blocks, the (partial) last block, blocks inside the window, and block 0 only until ``nsel`` later climbers are seen."""
    gen, out = torch.Generator().manual_seed(seed + 1), []
    for sl in kv:
        nb, per = -(-sl // bs), []
        for h in range(HEADS):
            climbs = [b < nsel or h == 1 or b == nb - 1 or bool(torch.rand(1, generator=gen) < 0.5) for b in range(nb)]
            low = torch.randperm(nb - sum(climbs), generator=gen).tolist()
            high = iter(range(nb - sum(climbs), nb))
            per.append([next(high) if up else low.pop() for up in climbs])
        out.append(per)
    return out


def margins_hold(c):
    """The builders' assertion: for every (row, head) the lowest taken block score is at least 4 x the highest one not taken."""
    for row, seq, _, t_kv, _ in rows_of(c):
        scores = []
        taken = row_weights(c, row, seq, t_kv, scores_out=scores)[1] if t_kv > 0 else []
        for h, chosen in enumerate(taken):
            rest = np.delete(scores[h], chosen)
            if rest.size and chosen and scores[h][chosen].min() < 4 * rest.max():
                return False
    return True


def selections(c):
    """Which of the three selections occur in some (row, head): the last, partial block taken; a taken block other than block 0
    overlapping the window; block 0 not taken — and which of them the geometry allows at all."""
    bs, nsel, ws = (c["cfg"][n] for n in ("block_size", "num_selected_blocks", "window_size"))
    seen = dict(partial=False, window=False, not_zero=False)
    can = dict(partial=False, window=False, not_zero=False)
    for row, seq, _, t_kv, _ in rows_of(c):
        if t_kv < c["cfg"]["compress_ratio"] or nsel == 0:
            continue
        nb = -(-t_kv // bs)
        groups_end = t_kv // c["cfg"]["compress_ratio"] * c["cfg"]["compress_ratio"]
        can["partial"] |= t_kv % bs != 0 and (groups_end > (nb - 1) * bs or nb <= nsel)     # without a complete group it scores 0
        can["window"] |= ws > 0 and nb > 1
        can["not_zero"] |= -(-(t_kv // c["cfg"]["compress_ratio"] * c["cfg"]["compress_ratio"]) // bs) > nsel   # blocks with a complete group
        for chosen in row_weights(c, row, seq, t_kv)[1]:
            seen["partial"] |= t_kv % bs != 0 and nb - 1 in chosen
            seen["window"] |= any(b > 0 and min((b + 1) * bs, t_kv) > t_kv - ws for b in chosen)
            seen["not_zero"] |= 0 not in chosen
    return seen, can


@functools.lru_cache(maxsize=None)
def geometry(op, t, dim, dtype, family, page=None, causal=True, many=None, most=None, seed=0):
    """The leg- and period-independent part of a case: sizes, query, key and scale.  Graded: ``K[t] = level[t // bs] step q_h /
    (scale |q_h|^2)`` at the smallest ``step`` (a multiple of 1/4) at which `margins_hold`, and the three selections occur."""
    cut, most = most is not None, most or (graded_most(t) if family == "graded" else None)   # cut: the CPU tests' short cases
    sizes = decode_lens(t, page, most) if op == "decode" else prefill_seqs(t, page, many and min(many, most or many), most or MAX_KEYS)
    query, key, qh, qq, scale, kv = _inputs(op, t, dim, dtype, sizes, seed)
    g = dict(op=op, t=t, dim=dim, dtype=dtype, family=family, page=page, causal=causal, sizes=sizes, query=query, key=key, qh=qh,
             qq=qq, scale=scale, kv=kv, cfg=cfg_of(t), step=None)
    if op == "prefill":
        g["seqs"] = sizes
    else:
        g["lens"] = torch.tensor(kv, dtype=torch.int32)
    if family == "graded":
        bs, levels = t[1], graded_levels(kv, t[1], t[2], seed)
        unit = qh.double() / (scale * qq[:, None])                      # a key of score 1 per head
        probe = dict(g, gate=torch.zeros(HEADS, dim, 3, dtype=dtype))
        for quarter in range(6, 41):
            g["step"] = quarter / 4
            for i, sl in enumerate(kv):
                for h in range(HEADS):
                    level = torch.tensor(levels[i][h], dtype=torch.float64).repeat_interleave(bs)[:sl]
                    key[i, :sl, h] = (level[:, None] * g["step"] * unit[h]).to(dtype)
            if margins_hold(dict(probe, key=key)):
                break
        else:
            raise AssertionError(f"{op} {t}: no step up to 10 separates the taken blocks by 4 x")
        seen, can = selections(dict(probe, key=key))
        assert cut or all(seen[n] for n in can if can[n]), (op, t, page, seen, can)
        g["selections"] = (seen, can)
    return g


@functools.lru_cache(maxsize=None)
def case(op, t, dim, dtype, family, leg, period, page=None, causal=True, many=None, most=None):
    """One pin case, in the layout of `nsa_golden.build` / `nsa_prefill_golden.build` (so their `model`, `paged` and `run`
    take it): ``period`` is ``D`` or ``D - 1``."""
    g = geometry(op, t, dim, dtype, family, page, causal, many, most)
    gate = torch.stack([sign * 16.0 * g["qh"].double() / g["qq"][:, None] for sign in LEGS[leg]], dim=-1).to(dtype)
    c = dict(g, leg=leg, period=period, gate=gate, value=_value(g["kv"], period, dim, dtype),
             lens=torch.tensor(g["kv"], dtype=torch.int32))
    if op == "prefill":
        cu = lambda j: torch.tensor([0] + [s[j] for s in g["sizes"]], dtype=torch.int32).cumsum(0).int()  # noqa: E731
        c.update(seqs=g["sizes"], cu_q=cu(0), cu_kv=cu(1))
    c["out64"] = G.model(c) if op == "decode" else GP.model(c)
    return c


def cases(op, t, dim, dtype, page=None, causal=True, many=None):
    return [case(op, t, dim, dtype, family, leg, period, page, causal, many)
            for family, legs in FAMILY_LEGS.items() if family == "equal" or t[2] > 0          # nsel 0: nothing to grade
            for leg in legs for period in (dim, dim - 1)]


def name_of(c):
    return (f"{c['op']} {c['t']} d{c['dim']} {str(c['dtype'])[6:]} page {c['page']}{'' if c['causal'] else ' not causal'} "
            f"{c['family']}/{c['leg']}/P{c['period']}")


def holed(c, page, hole):
    """K / V of a paged case whose table turns -1 at ``hole = (sequence, page index)``: zero rows from that key on."""
    key, value = c["key"].clone(), c["value"].clone()
    key[hole[0], hole[1] * page:], value[hole[0], hole[1] * page:] = 0, 0
    return key, value


def widen(table, width):
    """The table padded with -1 columns to ``width`` (the capacity ``page * width`` is what the prefill launch is planned on)."""
    if width is None or table.shape[1] >= width:
        return table
    return torch.cat([table, torch.full((table.shape[0], width - table.shape[1]), -1, dtype=table.dtype)], dim=1)


def run_decode(op, c, page, device="cpu", hole=None, **kw):
    """Case ``c`` through a decode op (contiguous for ``page`` None) at the case's ``softmax_scale``."""
    op = G.with_gate(op, c, device)
    if page is None:
        return op(*(x.to(device) for x in (c["query"], c["key"], c["value"], c["lens"])), c["scale"], **kw)
    kc, vc, table = G.paged(c, page, hole)
    return op(*(x.to(device) for x in (c["query"], kc, vc, c["lens"], table)), c["scale"], **kw)


def run_prefill(op, c, page, width=None, device="cpu", hole=None):
    """Case ``c`` through a prefill op: packed contiguous K/V for ``page`` None, else caches and a table of ``width`` columns."""
    op = G.with_gate(op, c, device)
    if page is None:
        key, value = (torch.cat([x[i, :kv] for i, (_, kv) in enumerate(c["seqs"])]) for x in (c["key"], c["value"]))
        return op(*(x.to(device) for x in (c["query"], key, value, c["cu_q"])), c["scale"])
    kc, vc, table = G.paged(c, page, hole)
    return op(*(x.to(device) for x in (c["query"], kc, vc, c["cu_q"], widen(table, width))), c["scale"],
              cu_total_seq_lens=c["cu_kv"].to(device))


def bound_of(c, out64):
    """The project's bound: ``u |out64| + 2^-12 max|V|``."""
    return UNIT[c["dtype"]] * out64.abs() + 2.0 ** -12 * AMP


def compare(got, c, out64=None, key=None, most=4):
    """(largest |err| / bound, failures, the set of (row, head, channel) beyond the bound).  A failure names (op, configuration, sequence, row, head, channel), the keys
    ``t = channel (mod P)`` of that row and the branches each is visible in (c / s / w), for the first ``most`` elements."""
    out64 = c["out64"] if out64 is None else out64
    got = got.detach().cpu().double()
    assert got.shape == out64.shape and not torch.isnan(got).any(), name_of(c)
    ratio = (got - out64).abs() / bound_of(c, out64)
    bad = (ratio > 1.0).nonzero().tolist()
    where = {row: (seq, t, t_kv) for row, seq, t, t_kv, _ in rows_of(c)}
    failures = []
    for row, h, ch in bad[:most]:
        seq, t, t_kv = where[row]
        open_gate = dict(c, gate=torch.zeros_like(c["gate"]))                      # visibility, whatever the leg's gate
        w = row_weights(open_gate, row, seq, t_kv, key=key)[0][:, h] if t_kv > 0 else np.zeros((3, 0))
        keys = [f"{k}:{''.join(b for b, x in zip('csw', w[:, k]) if x > 0) or '-'}" for k in range(ch, t_kv, c["period"])] if ch < c["period"] else []
        failures.append(f"{name_of(c)}: sequence {seq} row {t} head {h} channel {ch}: got {got[row, h, ch]:.6f} want "
                        f"{out64[row, h, ch]:.6f} ({ratio[row, h, ch]:.2f} x bound), {t_kv} keys seen, keys of the channel "
                        f"{' '.join(keys) or 'none'}")
    return float(ratio.max()) if ratio.numel() else 0.0, failures, {(r, h, ch) for r, h, ch in bad}


def edge_keys(c, w, taken, t_kv, leg):
    """The keys of a (row, head) at which the probed branch begins or ends."""
    cr, bs, ws = (c["cfg"][n] for n in ("compress_ratio", "block_size", "window_size"))
    if c["op"] == "prefill" and 0 < t_kv < cr:
        cr, bs = 1, max(bs, t_kv)
    if leg == "compressed":
        return {t_kv // cr * cr - 1} - {-1}
    if leg == "window":
        return {max(0, t_kv - ws), t_kv - 1} if ws > 0 else set()
    return {k for b in taken for k in (b * bs, min((b + 1) * bs, t_kv) - 1)}


def sensitivity(c):
    """The sensitivity condition of a single-branch case: ``8 w_t >= 2 bound`` at the key's channel.  Answers (edge keys that
    fall short, share of the remaining visible (row, head, key) triples that fall short)."""
    branch, short_edges, short, rest = BRANCH[c["leg"]], [], 0, 0
    bound = bound_of(c, c["out64"]).numpy()
    for row, seq, t, t_kv, _ in rows_of(c):
        if t_kv <= 0:
            continue
        w, taken = row_weights(c, row, seq, t_kv)
        for h in range(HEADS):
            ok = AMP * w[branch, h] >= 2.0 * bound[row, h, np.arange(t_kv) % c["period"]]
            seen = w[branch, h] > 0
            edges = sorted(k for k in edge_keys(c, w, taken[h], t_kv, c["leg"]) if seen[k])
            short_edges += [(seq, t, h, k) for k in edges if not ok[k]]
            seen[edges] = False
            short, rest = short + int((seen & ~ok).sum()), rest + int(seen.sum())
    return short_edges, short / max(rest, 1)
