"""The visible key set of every paged attention kernel, key by key, on every launch form.

The parity tests of this family compare random data with a 16-bit golden at 2e-2, which cannot see one key dropped, added or
counted twice among hundreds.  Here the inputs of tests/visibility.py make the output a read-out of the keys each row attended:
the visibility map (exact 0 for an invisible key, ``storage(1 / n)`` within 1 ulp for a visible one, every key position of every
sequence probed) and the selector (one key wins; 4 ulp of the storage type at 1.0).  The expectation is the definition
(`oracle.paged.window_mask`), tied to the ten goldens by tests/test_visibility_golden.py.  A failure names (sequence, row, head, key).

The selector's targets are every row's own causal and window edges and both sides of EVERY multiple of the 16-token tile and of
the page that some row of the sequence sees (`visibility.selector_plan`): every chunk, int8 step, prefill tile and key-slice edge of
a launch is one of them, and launches go on until each has met a head that probes it.

Each case forces its launch form with the switches, asserts the launch history it expects, and makes every call twice (same bits).
Sizes come from the code: 16-token decode tiles (DEC_TILE; the int8 kernel steps by two of them), 128-token minimum chunks
(decode_chunk_tokens, decode_seq_chunk), 16 // G steps per n-step block, 128 // G query rows and 64 keys per prefill block and
tile (PF_KEYS); a prefill key slice holds at least 8 tiles, so at <= 1024 keys a split launch cuts a block in two at the most.

Resolution of the row sum: 1 / n resolves n +- 1 by >= 2 ulp for n <= 127 in bf16 and n <= 1023 in fp16.  The window cases run
in the type noted beside each (``WINDOWS``); the unwindowed cases hold rows of n <= 127 (short sequences, early prefill rows)
beside the long ones, and every one of them also runs in fp16 on some geometry.

A page larger than the context (2048 tokens) runs with ``max_total_seq_len`` = the longest row, so that the launch takes the form
the case is about; one leg per kernel runs it without, on the 16 chunks the table's capacity plans.

Left out, by name, because the operators document them as unsupported: groups other than 1, 2, 4, 8 on the vector-unit decode
kernel and on the prefill kernels; head dims other than 64 / 128 on the 16-bit matrix-core decode kernel; `compute_dtype=int8`."""
import pytest
import torch

import visibility as V
from hip_utils import DEV, hip_cls, switch_env
from visibility import Case

pytestmark = pytest.mark.gpu
BF16, F16 = torch.bfloat16, torch.float16
SEEN, WORST = set(), {}                                  # launch histories seen; per operator [map ulp, selector |err|]


class Tagged:
    """``op`` with every call checked against the launch history it must leave."""

    def __init__(self, op, want, hint=None):
        self.op, self.want = op, want
        self.kw = {} if hint is None else dict(max_total_seq_len=hint)

    def forward(self, *args, **kw):
        from mojo_opset_amd.backends.hip import lib

        lib.launch_history(clear=True)
        out = self.op.forward(*args, **kw, **self.kw)
        torch.cuda.synchronize()
        got = lib.launch_history()
        assert got == self.want, (got, self.want)
        SEEN.add(got)
        return out


def run(case, env, want):
    env = dict(env)
    no_hint = env.pop("NO_HINT", False)
    # the selector's targets: both sides of every multiple of the 16-token tile and of the page that a row sees — chunks (whole
    # tiles, decode_seq_chunk), the int8 kernel's 32-token steps, the prefill kernel's 64-key tiles and its key slices (whole
    # tiles) all end on a multiple of 16
    strides = (16, case.page)
    with switch_env(**env):
        # a page larger than every context: the table's capacity says nothing about the lengths, so the caller's bound sizes the
        # launch, as it would in use (the bound is the longest row: nothing is truncated)
        hint = max(case.kv_lens) if case.kind != "prefill" and case.page > max(case.kv_lens) and not no_hint else None
        op = Tagged(case.make(hip_cls(case.op)), want, hint)
        worst = WORST.setdefault(case.op, [0.0, 0.0])
        for i, family in enumerate((V.MAP, V.SELECTOR)):
            failures, err = V.run_family(case, family, op, device=DEV, strides=strides, repeat=True)
            worst[i] = max(worst[i], err)
            print(f"{case.op} {family}: worst {err:.3g} {'ulp' if i == 0 else 'abs'}  [{want}]")
            assert not failures, f"{family} {env} {case}\n" + V.report(failures)


def ident(v):
    if isinstance(v, Case):
        win = "" if v.op not in V.WINDOW_OPS else f"-g{v.glob}-l{v.local}"
        return f"{v.op[4:]}-{str(v.dtype)[6:]}-{v.hq}x{v.hkv}x{v.d}-p{v.page}-{v.layout}{win}{'-holes' if v.holes else ''}"
    if isinstance(v, dict):
        return ",".join(f"{k[9:] if k.startswith('MOJO_HIP_') else k}={x}" for k, x in v.items()) or "default"
    return None


# (glob, local, dtype): the type in which the row sum of every row resolves n +- 1 (n <= glob + local + 1, <= 127 for bf16)
WINDOWS = [(None, 0, BF16), (1, 1, BF16), (4, 15, BF16), (16, 16, F16), (17, 17, BF16), (4, 63, BF16), (16, 64, F16),
           (17, 65, BF16), (None, 127, F16), (1, 127, F16), (16, None, BF16),
           (100, 63, F16),                               # overlapping at the lengths below (lo < glob): n = len <= 1023
           (4, 2000, F16)]                               # a window wider than every row

# ---- decode -----------------------------------------------------------------------------------------------------------
# (Hq, Hkv, D, page, layout, dtype); the page of 2048 tokens is larger than every context here
MFMA_GEOMS = [(8, 2, 128, 16, "AABB", BF16), (8, 1, 128, 32, "ABAB", F16), (4, 4, 64, 16, "ABAB", BF16),
              (4, 2, 64, 128, "AABB", F16), (6, 2, 128, 2048, "ABAB", BF16), (16, 1, 64, 16, "AABB", F16)]     # G 4 8 1 2 3 16
VALU_GEOMS = [(8, 2, 128, 16, "AABB", BF16), (8, 1, 96, 32, "ABAB", F16), (4, 4, 64, 128, "ABAB", BF16),
              (4, 2, 128, 2048, "AABB", F16), (8, 2, 96, 16, "ABAB", BF16), (4, 2, 128, 20, "AABB", BF16)]     # G 4 8 1 2 4 2
# (the vector-unit kernel takes pages of any multiple of 4 tokens: 20 is no power of two, so pages are found by division)
KV8_GEOMS = [(8, 2, 128, 16, "AABB", BF16), (8, 1, 64, 32, "ABAB", F16), (6, 2, 96, 128, "AABB", BF16),
             (4, 4, 80, 16, "ABAB", F16), (16, 1, 128, 1024, "AABB", BF16), (4, 2, 128, 48, "ABAB", F16)]     # G 4 8 3 1 16 2
# 1, tile - 1, tile, tile + 1, chunk - 1, chunk, chunk + 1, an empty row, a ragged rest (capacity 1008: 8 chunks of 128 tokens)
LENS = (1, 15, 16, 17, 127, 128, 129, 0, 1000, 513)
# the paired form: four 128-token chunks, batch >= 2 (an odd batch: the middle row has no partner)
PAIRED_LENS = (127, 128, 129, 511, 512, 1, 0, 300, 17)
# (form, switches, lengths): CHUNK=16 cuts a row into one-tile chunks — more than 8 of them take the grouped launch on the
# matrix-core kernel and the split one on the vector units
# one wave walks a whole row of up to 64 tiles: every round of the tile ring, and the matrix-core kernel's change of page-id window
# behind sub-tile 60 (token 960), with the row ending on, just behind and well behind it
LONG_LENS = (1000, 1024, 960, 961, 976, 977, 17, 0)
LONG = ("fused", dict(MOJO_HIP_DECODE_CHUNK="1024"), LONG_LENS)
FORMS = [("fused", {}, LENS), ("paired", {}, PAIRED_LENS), ("many", dict(MOJO_HIP_DECODE_CHUNK="16"), LENS),
         ("split+merge", dict(MOJO_HIP_DECODE_FUSE="0"), LENS), LONG]


def geom_kw(g):
    return dict(hq=g[0], hkv=g[1], d=g[2], page=g[3], layout=g[4], dtype=g[5])


def decode_tag(mfma, form, swa=False):
    form = {"many": "grouped+merge" if mfma else "split+merge"}.get(form, form)
    return f"decode_{'mfma' if mfma else 'valu'}:{form}:nt{':swa' if swa else ''}"


def decode_gqa_cases():
    out = []
    for mfma, geoms in ((1, MFMA_GEOMS), (0, VALU_GEOMS)):
        for gi, g in enumerate(geoms):
            for fi, (form, env, lens) in enumerate(FORMS):
                if form == "paired" and g[3] & (g[3] - 1):
                    continue                     # (four chunks need a capacity of 512 tokens: whole pages of a power of two)
                case = Case("MojoPagedDecodeGQA", "decode", lens, seed=gi * 4 + fi, **geom_kw(g))
                out.append((case, dict(env, MOJO_HIP_DECODE_MFMA=str(mfma)), decode_tag(mfma, form)))
        # the page larger than the context WITHOUT the caller's bound: the launch is sized on the table's capacity, one page of
        # 2048 tokens, so it plans 16 chunks of 128 tokens (the grouped launch, on the vector units the split one)
        g = next(g for g in geoms if g[3] == 2048)
        case = Case("MojoPagedDecodeGQA", "decode", LENS, seed=9, **geom_kw(g))
        out.append((case, dict(MOJO_HIP_DECODE_MFMA=str(mfma), NO_HINT=True), decode_tag(mfma, "many")))
        # holes: keys behind the first negative id count in n and read as zero K / V
        g = geoms[0]
        for form, env, lens in (FORMS[0], FORMS[2], FORMS[3]):
            case = Case("MojoPagedDecodeGQA", "decode", (1000, 300, 40, 17), holes=((0, 40), (1, 1), (2, 2)), seed=7, **geom_kw(g))
            out.append((case, dict(env, MOJO_HIP_DECODE_MFMA=str(mfma)), decode_tag(mfma, form)))
    return out


def swa_lens(glob, local):
    """Rows at, one short of and one past the window's size, around the tile, and long ones whose gap spans whole pages."""
    w = min(local if local is not None else 0, 400)
    lens = [1, 16, 17, w + 1, w + 2, w + 17, (glob or 0) + w + 1, 300, 1000, 0]
    return tuple(dict.fromkeys(min(n, 1000) for n in lens))


def decode_swa_cases():
    out = []
    legs = [(1, "fused", {}), (0, "fused", {}), (1, "many", dict(MOJO_HIP_DECODE_CHUNK="16")), (0, "many", dict(MOJO_HIP_DECODE_CHUNK="16")),
            (1, "split+merge", dict(MOJO_HIP_DECODE_FUSE="0")), (0, "split+merge", dict(MOJO_HIP_DECODE_FUSE="0"))]
    for wi, (glob, local, dtype) in enumerate(WINDOWS):
        for li, (mfma, form, env) in enumerate(legs):
            g = (MFMA_GEOMS if mfma else VALU_GEOMS)[(wi + li) % 4]
            # the launch is sized on the window (decode_swa_cap): more than 8 one-tile chunks only past 128 visible tokens
            span = -(-(glob or 0) // 16) * 16 + (local + 16 if local is not None else 0)
            if form == "many" and min(span, 1008) <= 128:
                continue                                                           # (it would be the fused leg again)
            case = Case("MojoPagedDecodeSWA", "decode", swa_lens(glob, local), glob=glob, local=local, seed=wi,
                        **dict(geom_kw(g), dtype=dtype))
            out.append((case, dict(env, MOJO_HIP_DECODE_MFMA=str(mfma)), decode_tag(mfma, form, True)))
    for mfma, geoms in ((1, MFMA_GEOMS), (0, VALU_GEOMS)):                       # a window wider than the row, one wave per row
        for gi in (0, 2):
            case = Case("MojoPagedDecodeSWA", "decode", LONG_LENS, glob=4, local=2000, seed=gi, **dict(geom_kw(geoms[gi]), dtype=F16))
            out.append((case, dict(LONG[1], MOJO_HIP_DECODE_MFMA=str(mfma)), decode_tag(mfma, "fused", True)))
    return out


def kv8_tag(form, swa=False, nstep=False):
    return f"decode_mfma:{form}:nt:kv8{':swa' if swa else ''}{':nstep' if nstep else ''}"


def decode_kv8_cases():
    out = []
    for gi, g in enumerate(KV8_GEOMS):
        for form, env, lens in (("fused", {}, LENS), ("split+merge", dict(MOJO_HIP_DECODE_FUSE="0"), LENS), LONG):
            case = Case("MojoPagedDecodeGQAWithKVDequant", "decode", lens, seed=gi, **geom_kw(g))
            out.append((case, env, kv8_tag(form)))
    for wi, (glob, local, dtype) in enumerate(WINDOWS):
        form, env = (("fused", {}), ("split+merge", dict(MOJO_HIP_DECODE_FUSE="0")))[wi % 2]
        g = KV8_GEOMS[wi % len(KV8_GEOMS)]
        case = Case("MojoPagedDecodeSWAWithKVDequant", "decode", swa_lens(glob, local), glob=glob, local=local, seed=wi,
                    **dict(geom_kw(g), dtype=dtype))
        out.append((case, env, kv8_tag(form, True)))
    return out


@pytest.mark.parametrize("case,env,want", decode_gqa_cases() + decode_swa_cases() + decode_kv8_cases(), ids=ident)
def test_decode(case, env, want):
    run(case, env, want)


# ---- n-step -----------------------------------------------------------------------------------------------------------
# (S, Hq, Hkv, D, page, layout): one block of 16 // G steps — full (4 x 4), half empty (2 x 8), twelve columns (4 x 3) —, two blocks
# (G 8, S 3), MHA (sixteen steps a block), and S = 1, the single-step op
NSTEP_GEOMS = [(4, 8, 2, 128, 16, "AABB"), (2, 8, 1, 64, 32, "ABAB"), (3, 8, 1, 128, 16, "AABB"), (4, 6, 2, 64, 128, "ABAB"),
               (3, 4, 4, 64, 16, "AABB"), (1, 8, 2, 128, 16, "ABAB")]
NSTEP_WINDOWS = [(None, None, BF16), (4, 5, BF16), (None, 0, BF16), (2, None, BF16), (16, 20, F16), (4, 63, BF16), (17, 65, BF16),
                 (1, 127, F16), (100, 63, F16)]


def nstep_lens(steps):
    """Lengths across the tile and the int8 kernel's 32-token step, ``len == S``, ``0 < len < S`` (steps that see no key store
    zeros), an empty row, and rows of several chunks."""
    return tuple(dict.fromkeys((16, 17, 18, 19, 33, 34, 64, 65, steps, 1, 2, 0, 130, 300, 1000)))


def nstep_cases():
    out = []
    for op, kv8 in (("MojoPagedDecodeNstepSWA", False), ("MojoPagedDecodeNstepSWAWithKVDequant", True)):
        tag = (lambda form, swa: kv8_tag(form, False, True)) if kv8 else (lambda form, swa: f"decode_mfma:{form}:nt:nstep")
        single = (lambda mfma, swa: kv8_tag("fused", swa)) if kv8 else (lambda mfma, swa: decode_tag(mfma, "fused", swa))
        for wi, (glob, local, dtype) in enumerate(NSTEP_WINDOWS):
            swa = glob is not None or local is not None
            for gi in (wi % 5, (wi + 2) % 5):
                steps, hq, hkv, d, page, layout = NSTEP_GEOMS[gi]
                case = Case(op, "nstep", nstep_lens(steps), steps=steps, hq=hq, hkv=hkv, d=d, page=page, layout=layout,
                            glob=glob, local=local, dtype=dtype, seed=wi)
                form, env = (("fused", {}), ("split+merge", dict(MOJO_HIP_DECODE_FUSE="0")))[(wi + gi) % 2]
                out.append((case, dict(env, MOJO_HIP_DECODE_MFMA="1"), tag(form, swa)))
            # the composed route: S single-step launches on the lengths len - (S - 1 - j)
            steps, hq, hkv, d, page, layout = NSTEP_GEOMS[wi % 3]
            if wi % 3 == 0 or kv8:
                case = Case(op, "nstep", nstep_lens(steps), steps=steps, hq=hq, hkv=hkv, d=d, page=page, layout=layout,
                            glob=glob, local=local, dtype=dtype, seed=wi + 50)
                out.append((case, dict(MOJO_HIP_DECODE_MFMA="0"), "|".join([single(0, swa)] * steps)))
        # more than 8 one-tile chunks: the grouped launch of the 16-bit n-step kernel
        if not kv8:
            case = Case(op, "nstep", nstep_lens(4), steps=4, seed=60)
            out.append((case, dict(MOJO_HIP_DECODE_MFMA="1", MOJO_HIP_DECODE_CHUNK="16"), tag("grouped+merge", False)))
        # S = 1 is the single-step op
        steps, hq, hkv, d, page, layout = NSTEP_GEOMS[5]
        for glob, local in ((None, None), (4, 15)):
            case = Case(op, "nstep", nstep_lens(1), steps=1, hq=hq, hkv=hkv, d=d, page=page, layout=layout, glob=glob, local=local,
                        seed=70)
            out.append((case, dict(MOJO_HIP_DECODE_MFMA="1"), single(1, glob is not None)))
    return out


@pytest.mark.parametrize("case,env,want", nstep_cases(), ids=ident)
def test_nstep(case, env, want):
    run(case, env, want)


# ---- prefill ----------------------------------------------------------------------------------------------------------
PREFILL_GEOMS = [(4, 4, 64, 16, "ABAB", BF16), (4, 2, 128, 32, "AABB", F16), (8, 2, 96, 16, "ABAB", BF16),
                 (8, 1, 128, 128, "AABB", F16), (8, 2, 64, 12, "AABB", BF16)]                                # G 1 2 4 8 4
# (pages of 12 tokens — any multiple of 4 is taken — have no fast staging: the general one runs whatever the switch says; the
# windowed int8 op wants pages of a multiple of 16 tokens, so the window cases walk the first four geometries)
# (MOJO_HIP_PREFILL_KSPLIT, MOJO_HIP_PREFILL_FAST_STAGE); 16 slices are more than the key tiles of any block here
STAGINGS = [(1, 1), (3, 1), (4, 1), (16, 1), (1, 0), (3, 0), (4, 0), (16, 0)]


def prefill_lens(group, glob=None, local=None):
    """(kv_lens, q_lens): a query block (128 // G rows) less one row, whole, plus one row, and one row; a cached prefix of 0, of
    one key, one that ends inside a 64-key tile; 16 key tiles (the one length here a split launch cuts in two); an empty
    sequence.  With a window: a cached prefix long enough for a gap of several whole pages."""
    qb = 128 // group
    kv = [qb - 1, qb + 1, qb + 1 + 37, 300, 1024, 0]
    q = [qb - 1, qb, qb + 1, 1, 40, 0]
    if glob is not None or local is not None:
        kv.append(900)
        q.append(qb + 3)
    return tuple(kv), tuple(q)


def prefill_tag(ksplit, fast, swa, page=16):
    fast = fast and page >= 16 and not page & (page - 1)
    return f"prefill:default:{'fast' if fast else 'general'}_stage:ksplit{ksplit}{':swa' if swa else ''}"


def prefill_env(ksplit, fast):
    return dict(MOJO_HIP_PREFILL_KSPLIT=str(ksplit), MOJO_HIP_PREFILL_FAST_STAGE=str(fast))


def prefill_cases():
    out = []
    for op, kv8 in (("MojoPagedPrefillGQA", False), ("MojoPagedPrefillGQAWithKVDequant", True)):
        for gi, g in enumerate(PREFILL_GEOMS):
            for k in range(2):
                ksplit, fast = STAGINGS[(gi * 2 + k * 5) % 8]
                kv, q = prefill_lens(g[0] // g[1])
                holes = ((3, 5), (4, 33)) if (k == 1 and not kv8 and g[3] == 16) else ()
                case = Case(op, "prefill", kv, q, pad_tokens=3, holes=holes, seed=gi * 2 + k, **geom_kw(g))
                want = prefill_tag(ksplit, fast, False, g[3]) + ("|gather:kv8+prefill" if kv8 else "")
                out.append((case, prefill_env(ksplit, fast), want))
    for op, kv8 in (("MojoPagedPrefillSWA", False), ("MojoPagedPrefillSWAWithKVDequant", True)):
        for wi, (glob, local, dtype) in enumerate(WINDOWS):
            for k in range(2):
                g = PREFILL_GEOMS[(wi + 2 * k) % 4]
                ksplit, fast = STAGINGS[(wi * 3 + kv8 + 4 * k) % 8]
                kv, q = prefill_lens(g[0] // g[1], glob, local)
                case = Case(op, "prefill", kv, q, pad_tokens=3, glob=glob, local=local, seed=wi, **dict(geom_kw(g), dtype=dtype))
                want = prefill_tag(ksplit, fast, True) + ("|gather:kv8:swa+prefill" if kv8 else "")
                out.append((case, prefill_env(ksplit, fast), want))
    return out


@pytest.mark.parametrize("case,env,want", prefill_cases(), ids=ident)
def test_prefill(case, env, want):
    run(case, env, want)
    # padding rows behind the last sequence are zeros (the comparer checked them: `V.unpack` returns them as one more entry)


# ---- what the file as a whole must have seen ----------------------------------------------------------------------------
REQUIRED = (
    [f"decode_mfma:{f}:nt" for f in ("paired", "fused", "grouped+merge", "split+merge")]
    + [f"decode_valu:{f}:nt" for f in ("paired", "fused", "split+merge")]
    + [f"decode_{k}:{f}:nt:swa" for k in ("mfma", "valu") for f in ("fused", "split+merge")] + ["decode_mfma:grouped+merge:nt:swa"]
    + [kv8_tag(f, swa) for f in ("fused", "split+merge") for swa in (False, True)]
    + [f"decode_mfma:{f}:nt:nstep" for f in ("fused", "grouped+merge", "split+merge")]
    + [kv8_tag(f, False, True) for f in ("fused", "split+merge")]
    + [prefill_tag(k, fast, swa) for k in (1, 3, 4, 16) for fast in (0, 1) for swa in (False, True)]
    + [prefill_tag(k, fast, swa) + f"|gather:kv8{':swa' if swa else ''}+prefill" for k, fast in ((1, 1), (4, 0)) for swa in (False, True)])


def test_every_form_was_seen_and_the_worst_deviations():
    """Runs last in the file: the launch histories the cases above left and, per operator, the worst deviation they met."""
    for op, (ulp, err) in sorted(WORST.items()):
        print(f"{op}: map worst {ulp:.0f} ulp, selector worst |err| {err:.3e}")
    print("launch histories seen:\n  " + "\n  ".join(sorted(SEEN)))
    planned = {want for case, env, want in decode_gqa_cases() + decode_swa_cases() + decode_kv8_cases() + nstep_cases()
               + prefill_cases()}
    assert set(REQUIRED) <= planned, sorted(set(REQUIRED) - planned)
    if len(WORST) == 10:                                 # (the whole file ran, not a selection of it)
        assert planned == SEEN, sorted(planned ^ SEEN)
