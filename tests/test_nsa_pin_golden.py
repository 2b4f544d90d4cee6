"""The NSA pin without a GPU: the core goldens on the pin's inputs, the sensitivity condition for every case the GPU file runs, the comparer against deliberately wrong fp64 models, and a closed form of the
equal family against the model."""
import numpy as np
import pytest
import torch

import nsa_golden as G
import nsa_pin as P
import nsa_prefill_golden as GP
from mojo_opset_amd.core.acc import check_tol_diff

DECODE_IDS = ["-".join(map(str, d[0])) for d in P.DECODE]
PREFILL_IDS = ["-".join(map(str, d[0])) for d in P.PREFILL]


def prefill_cases(entry, paged, causal=True):
    t, dim, dtype, page, width, _, _ = entry
    many = None if width is None else page * width - 5
    return P.cases("prefill", t, dim, dtype, page if paged else None, causal, many if paged else None)


def gpu_cases(op, entry):
    """Every case tests/test_hip_nsa_pin.py runs for a grid entry."""
    if op == "decode":
        return P.cases("decode", *entry[:3], entry[3])
    return [c for causal in entry[5] for paged in (False, True) for c in prefill_cases(entry, paged, causal)]


# ---- 1. the core goldens on the pin's inputs -----------------------------------------------------------------------------------------
def golden_legs(c):
    """The window-alone and compressed-alone legs, where the gate switches the selection off.  Its selected and
    all-on legs are left out for the goldens: ``torch.sort(stable=True)`` happens to take the lower index among equal block
    scores, but the reference's ``topk`` does not promise it."""
    return c["family"] == "equal" and c["leg"] in ("window", "compressed")


@pytest.mark.parametrize("entry", P.DECODE, ids=DECODE_IDS)
def test_decode_goldens_on_the_pin_inputs(entry):
    t, dim, dtype, page = entry
    for c in P.cases("decode", t, dim, dtype, page):
        if not golden_legs(c) or c["period"] != dim:
            continue
        keep = list(range(0, len(c["kv"]), 3))                     # a reduced set of lengths
        sub = dict(c, **{n: c[n][keep] for n in ("query", "key", "value", "lens", "out64")})
        for pg in (None, page):
            op = (G.TorchDecodeNSA if pg is None else G.TorchPagedDecodeNSA)(P.HEADS, dim, **c["cfg"])
            got = P.run_decode(op, sub, pg)
            check_tol_diff(got.double(), sub["out64"], atol=1e-2, rtol=1e-2)


@pytest.mark.parametrize("entry", P.PREFILL, ids=PREFILL_IDS)
def test_prefill_goldens_on_the_pin_inputs(entry):
    t, dim, dtype, page, width, causals, _ = entry
    for causal in causals:
        for c in P.cases("prefill", t, dim, dtype, None, causal):
            if not golden_legs(c) or c["period"] != dim:
                continue
            for pg in (None, page):
                op = (GP.TorchPrefillNSA if pg is None else GP.TorchPagedPrefillNSA)(P.HEADS, dim, is_causal=causal, **c["cfg"])
                check_tol_diff(P.run_prefill(op, c, pg).double(), c["out64"], atol=1e-2, rtol=1e-2)


def graded_entries():
    return [("decode", e) for e in P.DECODE if e[0][2] > 0] + [("prefill", e) for e in P.PREFILL if e[0][2] > 0]


@pytest.mark.parametrize("op,entry", graded_entries(), ids=[f"{op}-" + "-".join(map(str, e[0])) for op, e in graded_entries()])
def test_goldens_on_the_graded_family(op, entry):
    """No ties here, so the goldens' selected branch is tied to the fp64 model.  Rows are cut to 6 selection blocks: the
    goldens round ``q . k`` to the storage type, an error of ``2^-9 |score|`` (bf16) that grows with the level, and at 60 blocks
    of (2, 4, 4, 9) it reaches 0.27 of a score, shifts the weights among the taken blocks by a quarter and leaves 1e-2 (0.067)
    without any block changing sides."""
    t, dim, dtype, page = entry[:4]
    for leg in ("selected", "all"):
        c = P.case(op, t, dim, dtype, "graded", leg, dim, most=6 * t[1])
        for pg in (None, page):
            if op == "decode":
                got = P.run_decode((G.TorchDecodeNSA if pg is None else G.TorchPagedDecodeNSA)(P.HEADS, dim, **c["cfg"]), c, pg)
            else:
                got = P.run_prefill((GP.TorchPrefillNSA if pg is None else GP.TorchPagedPrefillNSA)(P.HEADS, dim, **c["cfg"]), c, pg)
            check_tol_diff(got.double(), c["out64"], atol=1e-2, rtol=1e-2)


# ---- 2. the sensitivity condition and the selections that must occur ----------------------------------------------------------------
@pytest.mark.parametrize("op,entry", graded_entries(), ids=[f"{op}-" + "-".join(map(str, e[0])) for op, e in graded_entries()])
def test_the_three_selections_occur_in_every_graded_case(op, entry):
    """The builder asserts them; here they are named per GPU case.  What a geometry cannot show is stated: (2, 2, 64, 0) has no
    window; where `graded_most` cuts the rows to ``nsel >= nb`` blocks ((2, 2, 64, 0), (16, 16, 5, 100), (4, 64, 16, 512)) block 0
    is always taken."""
    for c in gpu_cases(op, entry):
        if c["family"] == "graded":
            seen, can = c["selections"]
            assert seen["partial"] or not can["partial"], P.name_of(c)    # (16, 16, 3, 40) not causal: a partial block has no group
            assert seen["window"] or entry[0][3] == 0, P.name_of(c)
            assert seen["not_zero"] or not can["not_zero"], P.name_of(c)
            assert can["not_zero"] or P.graded_most(entry[0]) < P.MAX_KEYS or (op == "prefill" and c["page"] is None), P.name_of(c)



@pytest.mark.parametrize("op,entry", [("decode", e) for e in P.DECODE] + [("prefill", e) for e in P.PREFILL],
                         ids=["decode-" + i for i in DECODE_IDS] + ["prefill-" + i for i in PREFILL_IDS])
def test_every_gpu_case_is_sensitive(op, entry):
    """Single-branch legs: no edge key falls short of ``8 w >= 2 bound`` and at most 5 % of the other visible keys do.  (The
    all-on leg checks the sum of the three and has no probed branch.)"""
    t = entry[0]
    for c in gpu_cases(op, entry):
        if c["leg"] != "all":
            short_edges, share = P.sensitivity(c)
            assert not short_edges and share <= 0.05, (P.name_of(c), short_edges[:5], share)


def test_the_lengths_sit_on_both_sides_of_every_edge():
    got = P.lengths(3, 48, 2, 50, 16)
    assert {0, 1, 2, 3, 4, 47, 48, 49, 50, 51, 96, 97, 15, 16, 17, 255, 256, 257} <= set(got) and max(got) >= 997
    assert max(P.decode_lens((4, 64, 16, 512), 256)) <= 512 and min(P.lengths(2, 2, 64, 0)) == 0


# ---- 3. the comparer flags a wrong model and names the key ----------------------------------------------------------------------------
def moved_keys(c, wrong, branch, key=None):
    """{(row, head): keys whose visibility in ``branch`` differs between the true and the wrong model}."""
    moved = {}
    for row, seq, _, t_kv, _ in P.rows_of(c):
        a = P.row_weights(c, row, seq, t_kv)[0][branch] > 0
        b = P.row_weights(c, row, seq, t_kv, wrong, key)[0][branch] > 0
        n = max(a.shape[1], b.shape[1])
        a, b = (np.pad(x, ((0, 0), (0, n - x.shape[1]))) for x in (a, b))
        for h in range(P.HEADS):
            if (a[h] != b[h]).any():
                moved[(row, h)] = set(np.flatnonzero(a[h] != b[h]).tolist())
    return moved


def flags_exactly(make, wrong, branch):
    """The true model is clean.  The wrong model is flagged in every (row, head) where it moves a key and in no other, and every
    moved key is flagged at its channel in the run of period D or of period D - 1 (two moved keys one period apart cancel in
    that period's run; only a key with such a partner in both runs may stay unflagged); the failure text names the channel."""
    rows, hit, moved = set(), set(), None
    for period in (make("dim"), make("dim") - 1):
        c = make(period)
        assert P.compare((P.out_of_weights(c)).to(c["dtype"]), c)[1] == []
        moved = moved_keys(c, wrong, branch)
        assert moved, (P.name_of(c), wrong, "moves no key")
        _, failures, bad = P.compare(P.out_of_weights(c, wrong), c, most=10 ** 6)
        rows |= {(row, h) for row, h, _ in bad}
        hit |= {(row, h, k) for (row, h), keys in moved.items() for k in keys if (row, h, k % period) in bad}
        assert all(f"channel {ch}:" in " ".join(failures) for _, _, ch in bad)
    assert rows == set(moved), (wrong, sorted(rows ^ set(moved)))
    for (row, h), keys in moved.items():           # a moved key that is flagged in neither run is cancelled in BOTH by other moved keys
        for k in keys:
            assert (row, h, k) in hit or all(any(o != k and (o - k) % period == 0 for o in keys) for period in (make("dim"), make("dim") - 1)), \
                (wrong, row, h, k)


DEC, PRE = P.DECODE[4], P.PREFILL[2]            # (4, 8, 3, 20) and the anchor (4, 32, 2, 48)


@pytest.mark.parametrize("wrong,leg", [("ws+1", "window"), ("ws-1", "window"), ("ceil groups", "compressed"), ("block short", "selected"),
                                       ("block long", "selected"), ("tie high", "selected"), ("one block fewer", "selected")])
def test_the_comparer_flags_a_wrong_decode_model_at_the_keys_it_moves(wrong, leg):
    t, dim, dtype, page = DEC
    flags_exactly(lambda p: dim if p == "dim" else P.case("decode", t, dim, dtype, "equal", leg, p, page), wrong, P.BRANCH[leg])


@pytest.mark.parametrize("wrong,leg", [("t_kv+1", "window"), ("t_kv-1", "window"), ("t_kv+1", "compressed"),
                                       ("short rows as decode", "compressed"), ("ws+1", "window"), ("block short", "selected"),
                                       ("tie high", "selected")])
def test_the_comparer_flags_a_wrong_prefill_model_at_the_keys_it_moves(wrong, leg):
    t, dim, dtype, page = PRE[:4]
    flags_exactly(lambda p: dim if p == "dim" else P.case("prefill", t, dim, dtype, "equal", leg, p, page), wrong, P.BRANCH[leg])


@pytest.mark.parametrize("op", ["decode", "prefill"])
def test_the_comparer_flags_keys_read_behind_a_hole(op):
    """The model of the holed table (zero K / V rows behind it) is clean; a model that reads the pages as if they were valid is
    flagged in the sequence with the hole and nowhere else."""
    if op == "decode":
        (t, at), entry = P.DECODE_HOLE, next(e for e in P.DECODE if e[0] == P.DECODE_HOLE[0])
        c = P.case("decode", t, entry[1], entry[2], "equal", "window", entry[1], entry[3])
        seq = len(c["kv"]) - 1
        want = G.model(c, *P.holed(c, entry[3], (seq, at)))
    else:
        (t, at), entry = P.PREFILL_HOLE, next(e for e in P.PREFILL if e[0] == P.PREFILL_HOLE[0])
        c, seq = P.case("prefill", t, entry[1], entry[2], "equal", "window", entry[1], entry[3]), 2
        want = GP.model(c, *P.holed(c, entry[3], (seq, at)))
    assert P.compare(want.to(c["dtype"]), c, out64=want)[1] == []
    _, failures, bad = P.compare(c["out64"], c, out64=want)
    rows = {row for row, s, _, t_kv, _ in P.rows_of(c) if s == seq and t_kv > at * entry[3]}
    assert bad and {row for row, _, _ in bad} == rows and f"sequence {seq} " in failures[0]


# ---- 4. a closed form of the equal family against the model -------------------------------------------------------------------------
@pytest.mark.parametrize("entry", P.DECODE, ids=DECODE_IDS)
def test_equal_family_closed_form(entry):
    """w_t = g0 / (C cr) [t < C cr] + g1 / n_sel_keys [t in blocks 0 ..] + g2 / min(ws, sl) [t >= sl - ws]: written down
    independently of `model_one` (a partial last block without a complete group scores 0 and loses to every full block)."""
    t, dim, dtype, page = entry
    cr, bs, nsel, ws = t
    for leg in P.LEGS:
        c = P.case("decode", t, dim, dtype, "equal", leg, dim - 1, page)
        g = [0.5] * 3 if leg == "all" else [float(s > 0) for s in P.LEGS[leg]]
        want = np.zeros(tuple(c["out64"].shape))
        for i, sl in enumerate(c["kv"]):
            if sl == 0:
                continue
            w, k = np.zeros(sl), np.arange(sl)
            n_c, nb = sl // cr * cr, -(-sl // bs)
            w[:n_c] += g[0] / max(n_c, 1)
            taken = range(min(nsel, nb))           # full blocks tie, the partial last block has fewer groups: lower indices win
            keys = np.concatenate([np.arange(b * bs, min((b + 1) * bs, sl)) for b in taken]) if len(taken) else np.arange(0)
            w[keys] += g[1] / max(keys.size, 1)
            if ws > 0:
                w[k >= sl - ws] += g[2] / min(ws, sl)
            for ch in range(dim - 1):
                want[i, :, ch] = P.AMP * w[ch::dim - 1].sum()
        assert np.abs(want - c["out64"].numpy()).max() < 1e-5, (P.name_of(c), np.abs(want - c["out64"].numpy()).max())


def test_the_weights_are_the_models():
    """`weights_one` and `nsa_golden.model_one` / `nsa_prefill_golden.model` are one definition: outputs agree to 1e-12."""
    for c in (P.case("decode", DEC[0], DEC[1], DEC[2], "equal", "all", 64, DEC[3]),
              P.case("prefill", PRE[0], PRE[1], PRE[2], "equal", "all", 63, PRE[3]),
              P.case("prefill", PRE[0], PRE[1], PRE[2], "equal", "all", 64, PRE[3], False)):
        assert (P.out_of_weights(c) - c["out64"]).abs().max() < 1e-12, P.name_of(c)
