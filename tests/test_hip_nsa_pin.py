"""The NSA pin on an MI355X: `HIPDecodeNSA` / `HIPPagedDecodeNSA` (csrc/nsa_decode.hip) and `HIPPrefillNSA` /
`HIPPagedPrefillNSA` (csrc/nsa_prefill.hip) against the fp64 model on inputs whose output is a read-out of the visible keys, on
every geometry of tests/nsa_pin.py and in every launch form.  The bound is the project's, ``u |out64| + 2^-12 max|V|``."""
import pytest
import torch

import nsa_golden as G
import nsa_pin as P
import nsa_prefill_golden as GP
from mojo_opset_amd.backends.hip import lib as L
from mojo_opset_amd.backends.hip.operators.nsa import HIPDecodeNSA, HIPPagedDecodeNSA, HIPPagedPrefillNSA, HIPPrefillNSA

pytestmark = pytest.mark.gpu
SEEN, PLANNED, WORST = set(), {}, {"decode": 0.0, "prefill": 0.0}
DECODE_IDS = ["-".join(map(str, d[0])) for d in P.DECODE]
PREFILL_IDS = ["-".join(map(str, d[0])) for d in P.PREFILL]


def judge(got, c, out64=None, key=None):
    ratio, failures, _ = P.compare(got, c, out64, key)
    WORST[c["op"]] = max(WORST[c["op"]], ratio)
    assert not failures, "\n".join(failures)
    return ratio


def decode_tag(num_splits, dim, cap):
    tiles = -(-cap // 16)
    return f"nsa_decode:fused:d{dim}" if num_splits == 1 else f"nsa_decode:split{min(num_splits, tiles)}:d{dim}"


@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
@pytest.mark.parametrize("entry", P.DECODE, ids=DECODE_IDS)
def test_decode_reads_exactly_the_visible_keys(entry, paged):
    t, dim, dtype, page = entry
    worst = 0.0
    for c in P.cases("decode", t, dim, dtype, page):
        op = (HIPPagedDecodeNSA if paged else HIPDecodeNSA)(P.HEADS, dim, **c["cfg"])
        pg = page if paged else None
        cap = page * (-(-max(c["kv"]) // page) + 2) if paged else max(c["kv"])
        forced = {}
        for num_splits in P.SPLITS:
            n = -(-max(c["kv"]) // 16) if num_splits == "tiles" else num_splits          # one-tile slices, empty for short rows
            got = P.run_decode(op, c, pg, "cuda", num_splits=n)
            tag = L.last_launch()
            SEEN.add(tag)
            if n is not None:
                assert tag == decode_tag(n, dim, cap), (P.name_of(c), n, tag)
                forced[tag] = got
            else:
                PLANNED.setdefault((t, paged), set()).add(tag)
                if tag in forced:
                    first = forced[tag]
                elif tag.startswith("nsa_decode:split1:"):               # (one slice cannot be forced: num_splits 1 is the fused form)
                    first = got
                else:
                    first = P.run_decode(op, c, pg, "cuda", num_splits=int(tag.split(":")[1][5:]))
                assert torch.equal(got, first), f"{P.name_of(c)}: the planned call ({tag}) differs from the forced call of its form"
            worst = max(worst, judge(got, c))
            assert torch.equal(P.run_decode(op, c, pg, "cuda", num_splits=n), got), f"{P.name_of(c)}: two calls of {tag} differ"
    print(f"decode {t} {'paged' if paged else 'contiguous'}: max |err| / bound = {worst:.3f}")


def run_prefill(op, c, page, width, hole=None):
    return P.run_prefill(op, c, page, width, "cuda", hole)


@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
@pytest.mark.parametrize("entry", P.PREFILL, ids=PREFILL_IDS)
def test_prefill_reads_exactly_the_visible_keys(entry, paged):
    t, dim, dtype, page, width, causals, waves = entry
    worst = 0.0
    for causal in causals:
        many = page * width - 5 if paged and width is not None else None
        for c in P.cases("prefill", t, dim, dtype, page if paged else None, causal, many):
            op = (HIPPagedPrefillNSA if paged else HIPPrefillNSA)(P.HEADS, dim, is_causal=causal, **c["cfg"])
            got = run_prefill(op, c, page if paged else None, width)
            tag = L.last_launch()
            SEEN.add(tag)
            assert tag == f"nsa_prefill:w{waves if paged else 4}:d{dim}", (P.name_of(c), tag)
            worst = max(worst, judge(got, c))
            if paged:                                                    # rows with t_kv <= 0 are exact zeros
                for row, _, _, t_kv, _ in P.rows_of(c):
                    assert t_kv > 0 or not got[row].any(), (P.name_of(c), row)
            assert torch.equal(run_prefill(op, c, page if paged else None, width), got), f"{P.name_of(c)}: two calls differ"
    print(f"prefill {t} {'paged' if paged else 'contiguous'}: max |err| / bound = {worst:.3f}")


@pytest.mark.parametrize("op", ["decode", "prefill"])
def test_a_table_that_turns_negative_inside_a_block_reads_zero_rows(op):
    """The table turns -1 on a page edge inside a selection block (decode: inside a group as well)."""
    if op == "decode":
        (t, at), (_, dim, dtype, page) = P.DECODE_HOLE, next(e for e in P.DECODE if e[0] == P.DECODE_HOLE[0])
        for c in P.cases("decode", t, dim, dtype, page):
            seq = len(c["kv"]) - 1
            key, value = P.holed(c, page, (seq, at))
            want = G.model(c, key, value)
            hip = HIPPagedDecodeNSA(P.HEADS, dim, **c["cfg"])
            for num_splits in (1, 5):
                judge(P.run_decode(hip, c, page, "cuda", (seq, at), num_splits=num_splits), c, want, key)
    else:
        (t, at), (_, dim, dtype, page, width, _, _) = P.PREFILL_HOLE, next(e for e in P.PREFILL if e[0] == P.PREFILL_HOLE[0])
        for c in P.cases("prefill", t, dim, dtype, page):
            key, value = P.holed(c, page, (2, at))
            judge(run_prefill(HIPPagedPrefillNSA(P.HEADS, dim, **c["cfg"]), c, page, width, (2, at)), c, GP.model(c, key, value), key)


def test_every_form_was_seen_and_the_worst_deviations():
    """Runs last: every planned launch form was taken when the whole file ran."""
    want = {f"nsa_decode:fused:d{d}" for d in (64, 128)} | {f"nsa_decode:split{n}:d{d}" for n in (2, 5) for d in (64, 128)}
    want |= {f"nsa_prefill:w4:d{d}" for d in (64, 128)} | {"nsa_prefill:w2:d64", "nsa_prefill:w1:d128"}
    want |= {decode_tag(-(-max(P.decode_lens(t, page)) // 16), dim, 1 << 20) for t, dim, _, page in P.DECODE}
    assert want <= SEEN, sorted(want - SEEN)
    assert len(PLANNED) == 2 * len(P.DECODE) and any(":split" in tag for tags in PLANNED.values() for tag in tags), PLANNED   # asked everywhere, and it split
    print(f"planned forms: {PLANNED}")
    print(f"forms seen: {sorted(SEEN)}\nworst |err| / bound: decode {WORST['decode']:.3f}, prefill {WORST['prefill']:.3f}")
