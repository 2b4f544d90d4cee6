"""The visible key set of the MLA kernels, key by key, on every route and launch form.

The parity tests of the MLA pair compare random-normal data at 1e-2 (4e-2 against the golden), which cannot see one key dropped,
leaked or counted twice among hundreds.  Here the inputs of tests/visibility_mla.py make the output a read-out of the keys each
row attended: the visibility map (exact 0 for an invisible key, ``storage(1 / n)`` within 1 ulp for a visible one, every key of
every sequence probed, the sink's one in the denominator of the even heads) and two selectors (one key wins; 4 ulp of the
storage type at 1.0), rope-coded — ``k_pe`` row ``s`` must meet latent row ``s`` — and nope-coded — the absorbed query GEMM, or
the decompressed ``K_nope``, per head.  The expectation is the definition, tied to the two goldens by
tests/test_visibility_mla_golden.py.  A failure names (sequence, row, head, key).

Every case forces its route with the switches, asserts the launch tag it expects in the launch history (by containment: the
history also holds the per-head GEMMs), and makes every call twice (same bits).  Sizes come from the code: the ``ps`` kernel walks
32-key tiles, ``oct`` and the general latent kernel 64-key tiles; a key split holds ``ceil(ceil(capacity / splits) / 64) * 64``
keys, capacity = page x table width (1024 tokens in the decode cases, so 5 splits leave the fifth without a key and 6 the
sixth); `mla_prefill_kernel` takes 128 query rows per block and 64-key tiles.  The selectors' targets are every row's own edges
(``p``, ``p + 1``, 0, ``n - 1``, both sides of its first hole) and both sides of EVERY multiple of 32, of 64 (every split edge is
one) and of the page; a page below 16 tokens is left out of the strides.

Lengths: 1, tile -+ 1 and tile (both tiles), split -+ 1 and split, an empty row, a ragged row of 1000 keys, and rows of
n <= 127.  Resolution of the row sum: 1 / n resolves n +- 1 by >= 2 ulp for n <= 127 in bf16 and n <= 1023 in fp16; every route
runs in both types.

The page-id window cases (one workgroup walks more than the 1024 / 4096 table entries its LDS window holds: page 1,
``MOJO_HIP_MLA_SPLITS=1``) hold rows of 1100 and 4200 keys.  At these lengths the map's 1 / n no longer resolves n +- 1 in
either type; its probes still read exactly 0 for a dropped key and 2 / n for a doubled one, and the selectors (11 and 13 code
bits) aim at both sides of the window boundary and of the tile edges around it.

Left out: the experiments-build kernels ``pp`` and ``pair``; non-causal prefill (raises); pages that are no power of two at
r = 512 (refused)."""
import dataclasses

import pytest
import torch

import visibility_mla as M
from hip_utils import DEV, hip_cls, switch_env
from visibility_mla import Case, default_splits, split_keys      # (sizes, as the host code computes them)

pytestmark = pytest.mark.gpu
BF16, F16 = torch.bfloat16, torch.float16
DECODE, PREFILL = "MojoPagedDecodeMLA", "MojoPagedPrefillMLA"
SEEN, WORST = set(), {}                                  # launch tags seen; per route [map ulp, rope |err|, nope |err|]
CAPACITY = 1024                                          # tokens the block table of a decode case can name
UNSET = dict(MOJO_HIP_MLA_KERNEL=None, MOJO_HIP_MLA_SPLITS=None, MOJO_HIP_MLA_DECODE=None, MOJO_HIP_MLA_PREFILL=None,
             MOJO_HIP_MLA_PREFILL_BYTES=None)
# (nope, rope, vd) by (r, rope) of the latent kernels; the three sets the decompressed prefill kernel is built for
R512 = dict(nope=128, rope=64, vd=128, r=512)
GENERAL = {64: dict(nope=96, rope=32, vd=128, r=64), 32: dict(nope=64, rope=32, vd=64, r=32),
           128: dict(nope=128, rope=64, vd=128, r=128), 256: dict(nope=128, rope=64, vd=128, r=256)}
DECOMPRESSED = [R512, GENERAL[32], GENERAL[64]]


class Tagged:
    """``op`` with every call checked against the launch tag it must leave (its parameters show through)."""

    def __init__(self, op, tag):
        self.op, self.tag = op, tag

    def __getattr__(self, name):
        return getattr(self.op, name)

    def forward(self, *args, **kw):
        from mojo_opset_amd.backends.hip import lib

        lib.launch_history(clear=True)
        out = self.op.forward(*args, **kw)
        torch.cuda.synchronize()
        got = lib.launch_history()
        assert self.tag in got, (got, self.tag)
        SEEN.add(self.tag)
        return out


def run(route, case, env, tag, strides=None, extra=(), groups=None, **call_kw):
    if strides is None:
        strides = (32, 64) + ((case.page,) if case.page >= 16 else ())
    with switch_env(**dict(UNSET, **env)):
        op = Tagged(case.make(hip_cls(case.op), DEV), tag)
        if groups:
            op.op.prefill_head_groups = groups
        worst = WORST.setdefault(route, [0.0, 0.0, 0.0])
        for i, family in enumerate(M.FAMILIES):
            failures, err = M.run_family(case, family, op, device=DEV, strides=strides, extra=extra, repeat=True, **call_kw)
            worst[i] = max(worst[i], err)
            print(f"{route} {family}: worst {err:.3g} {'ulp' if i == 0 else 'abs'}  [{tag}]")
            assert not failures, f"{family} {env} {case}\n" + M.report(failures)


def ident(v):
    if isinstance(v, Case):
        return (f"{v.kind}-{str(v.dtype)[6:]}-h{v.heads}-r{v.r}-p{v.page}{'-sink' if v.sink else ''}{'-holes' if v.holes else ''}"
                f"-n{max(v.kv_lens)}")
    if isinstance(v, dict):
        return ",".join(f"{k[9:] if k.startswith('MOJO_HIP_') else k}={x}" for k, x in v.items()) or "default"
    return v if isinstance(v, str) else None


def decode_lens(split, capacity=CAPACITY):
    """1, both tiles -+ 1, the split -+ 1, an empty row, a ragged long row, a row of n <= 127 off every edge."""
    want = [1, 31, 32, 33, 63, 64, 65, split - 1, split, split + 1, 0, 1000, 100]
    return tuple(dict.fromkeys(n for n in want if n <= capacity))


def holes_at(lens, page, keys):
    """``(sequence, logical page)`` of a hole at key position ``keys[b]`` (whole pages; page >= 1 and inside the sequence)."""
    out = []
    for b, key in keys:
        p = key // page
        if 1 <= p < -(-lens[b] // page):
            out.append((b, p))
    return tuple(out)


HOLE_LENS = (1000, 300, 40, 100, 17, 0, 700)


def decode_case(dims, heads, page, splits, dtype, sink, seed, holes=False, lens=None):
    """A decode case on a table of `CAPACITY` tokens and the splits its launch takes (``splits`` None: the default)."""
    pages = -(-CAPACITY // page)
    n, given = splits, lens
    for _ in range(2):                                   # (the default depends on the batch, the batch on the split's size)
        lens = given or (HOLE_LENS if holes else decode_lens(split_keys(pages * page, n or 4)))
        n = splits or default_splits(len(lens), heads, dims["r"], dims["rope"], pages * page)
    hs = holes_at(lens, page, ((0, 640), (1, 64), (2, 32), (3, 16), (6, 512))) if holes else ()
    return Case(DECODE, "decode", lens, heads=heads, page=page, dtype=dtype, sink=sink, seed=seed, holes=hs, table_pages=pages,
                **dims), n


def splits_env(splits):
    return {} if splits is None else dict(MOJO_HIP_MLA_SPLITS=str(splits))


# ---- 1. absorbed decode, r = 512 ------------------------------------------------------------------------------------------
# (kernel, switch, page): `oct` is forced at page 16 and taken by itself below 16 tokens a page (1: the smallest the op takes)
R512_KERNELS = [("ps", {}, 16), ("ps", {}, 64), ("oct", dict(MOJO_HIP_MLA_KERNEL="oct"), 16), ("oct", {}, 1)]


def r512_cases():
    out = []
    for ki, (kernel, env, page) in enumerate(R512_KERNELS):
        for si, splits in enumerate((None, 1, 2, 5)):
            heads = (8, 40, 128)[(ki + si) % 3]          # less than one wave of 16, no multiple of 16, two 64-head blocks
            dtype, sink = (BF16, F16)[(ki + si) % 2], bool((ki // 2 + si) % 2)
            case, n = decode_case(R512, heads, page, splits, dtype, sink, seed=ki * 4 + si)
            out.append((case, dict(env, **splits_env(splits)), f"mla512:{kernel}:splits{n}"))
    for ki, splits in ((0, 2), (2, None)):                # one hole case per kernel: the second split starts behind a hole
        kernel, env, page = R512_KERNELS[ki]
        case, n = decode_case(R512, 40, page, splits, (F16, BF16)[ki // 2], ki == 0, seed=20 + ki, holes=True)
        out.append((case, dict(env, **splits_env(splits)), f"mla512:{kernel}:splits{n}"))
    return out


@pytest.mark.parametrize("case,env,tag", r512_cases(), ids=ident)
def test_absorbed_decode_r512(case, env, tag):
    run("absorbed decode r512 " + tag.split(":")[1], case, env, tag)


# ---- 2. absorbed decode, the general kernel ---------------------------------------------------------------------------------
# pages: powers of two, and a multiple of 8 that is none (pages found by division)
GENERAL_PAGES = {64: 24, 32: 16, 128: 8, 256: 32}


def general_cases():
    out = []
    for ri, (r, dims) in enumerate(GENERAL.items()):
        for si, splits in enumerate((1, 3, 6)):
            heads, dtype, sink = (8, 24)[(ri + si) % 2], (BF16, F16)[(ri + si) % 2], bool((ri + si // 2) % 2)
            case, n = decode_case(dims, heads, GENERAL_PAGES[r], splits, dtype, sink, seed=ri * 3 + si)
            out.append((case, splits_env(splits), f"mla_latent:r{r}:splits{n}"))
    for r, splits, dtype in ((64, 3, F16), (256, None, BF16)):
        case, n = decode_case(GENERAL[r], 24, GENERAL_PAGES[r], splits, dtype, r == 64, seed=30 + r, holes=True)
        out.append((case, splits_env(splits), f"mla_latent:r{r}:splits{n}"))
    return out


@pytest.mark.parametrize("case,env,tag", general_cases(), ids=ident)
def test_absorbed_decode_general(case, env, tag):
    run("absorbed decode general", case, env, tag)


# ---- 3. the page-id window refill -------------------------------------------------------------------------------------------
def around(boundary):
    """Both sides of the window boundary and of the 32- and 64-key tile edges around it."""
    return tuple(t for m in (boundary - 64, boundary - 32, boundary, boundary + 32, boundary + 64) for t in (m - 1, m))


def window_cases():
    out = []
    for dtype in (BF16, F16):
        # `oct`: 1024 entries; rows that end on, just behind and well behind the window's last page, beside short ones
        case = Case(DECODE, "decode", (1100, 1024, 1025, 40, 0), heads=8, page=1, dtype=dtype, sink=dtype == F16, seed=40,
                    code_bits=11, **R512)
        out.append((case, dict(MOJO_HIP_MLA_SPLITS="1"), "mla512:oct:splits1", around(1024)))
        # the general kernel: 4096 entries
        case = Case(DECODE, "decode", (4200, 4097, 40, 0), heads=8, page=1, dtype=dtype, sink=dtype == BF16, seed=41,
                    code_bits=13, **GENERAL[64])
        out.append((case, dict(MOJO_HIP_MLA_SPLITS="1"), "mla_latent:r64:splits1", around(4096)))
    return out


@pytest.mark.parametrize("case,env,tag,extra", window_cases(), ids=ident)
def test_page_id_window_refill(case, env, tag, extra):
    run("page-id window refill " + tag.split(":")[0], case, env, tag, strides=(), extra=extra)


# ---- 4. absorbed prefill ----------------------------------------------------------------------------------------------------
def absorbed_prefill_cases():
    out = []
    absorbed = dict(MOJO_HIP_MLA_PREFILL="absorbed")
    # by the switch: several sequences, cached prefixes of 0, of 1 and one that ends inside a tile, an empty sequence, padding
    q, prefix = (40, 1, 20, 0, 5), (0, 1, 100, 0, 300)
    kv = tuple(a + b for a, b in zip(q, prefix))
    for dims, heads, page, splits, dtype, sink, tag in (
            (R512, 8, 16, 2, BF16, True, "mla512:ps:splits2"), (R512, 40, 8, 3, F16, False, "mla512:oct:splits3"),
            (GENERAL[64], 24, 16, 3, F16, True, "mla_latent:r64:splits3"), (GENERAL[256], 8, 32, 5, BF16, False, "mla_latent:r256:splits5")):
        case = Case(PREFILL, "prefill", kv, q, heads=heads, page=page, dtype=dtype, sink=sink, pad_tokens=3, seed=50, **dims)
        out.append((case, dict(absorbed, MOJO_HIP_MLA_SPLITS=str(splits)), tag))
    # by size: fewer than 16 query tokens, padding included (dimension sets the decompressed kernel is built for); the table
    # names 1024 tokens, so the default is four splits
    q, prefix = (3, 1, 5, 0, 2), (200, 0, 37, 0, 1)
    kv = tuple(a + b for a, b in zip(q, prefix))
    for dims, page, dtype, tag in ((R512, 16, F16, "mla512:ps:splits4"), (GENERAL[32], 16, BF16, "mla_latent:r32:splits4")):
        case = Case(PREFILL, "prefill", kv, q, heads=8, page=page, dtype=dtype, sink=dtype == BF16, pad_tokens=2, seed=51,
                    table_pages=CAPACITY // page, **dims)
        out.append((case, {}, tag))
    return out


@pytest.mark.parametrize("case,env,tag", absorbed_prefill_cases(), ids=ident)
def test_absorbed_prefill(case, env, tag):
    run("absorbed prefill", case, env, tag)


# ---- 5. decompressed prefill ------------------------------------------------------------------------------------------------
# a query block (128 rows) less one row, whole, plus one row, one row, 40 rows; cached prefixes of 0, of 1, one that ends inside a
# 64-key tile; a sequence of 1024 keys; an empty sequence; 3 padding rows
PF_Q = (127, 128, 129, 1, 40, 0)
PF_PREFIX = (0, 1, 37, 300, 984, 0)
PF_KV = tuple(a + b for a, b in zip(PF_Q, PF_PREFIX))


def decompressed_prefill_cases():
    out = []
    for di, dims in enumerate(DECOMPRESSED):
        heads, page = (8, 8, 16)[di], (16, 32, 16)[di]
        cached = Case(PREFILL, "prefill", PF_KV, PF_Q, heads=heads, page=page, pad_tokens=3, seed=60 + di, **dims)
        fresh = Case(PREFILL, "prefill", PF_Q, PF_Q, heads=heads, page=page, pad_tokens=3, seed=63 + di, **dims)
        one_seq = max(PF_KV) * heads * (dims["nope"] + dims["vd"]) * 2      # the decompressed image of the longest sequence
        forms = [("plain", cached, {}, {}), ("no-cu-kv", fresh, {}, dict(no_cu_kv=True)),
                 ("slices", cached, dict(MOJO_HIP_MLA_PREFILL_BYTES=str(one_seq)), dict(max_total_seq_len=max(PF_KV))),
                 ("groups", cached, {}, dict(groups=2)), ("hint", cached, {}, dict(max_total_seq_len=max(PF_KV)))]
        for fi, (form, case, env, kw) in enumerate(forms):
            dtype, sink = (BF16, F16)[(fi + di) % 2], bool((fi // 2 + di) % 2)
            out.append((form, dataclasses.replace(case, dtype=dtype, sink=sink), env, kw))
    return out


@pytest.mark.parametrize("form,case,env,kw", decompressed_prefill_cases(), ids=ident)
def test_decompressed_prefill(form, case, env, kw):
    run("decompressed prefill", case, env, "mla_prefill_attn", **kw)


# ---- 6. the golden-rounding decode route ------------------------------------------------------------------------------------
def golden_route_cases():
    out = []
    golden = dict(MOJO_HIP_MLA_DECODE="golden")
    for di, dims in enumerate(DECOMPRESSED):
        heads, page = (8, 8, 16)[di], (16, 32, 16)[di]
        one_seq = 1000 * heads * (dims["nope"] + dims["vd"]) * 2
        for holes in (False, True):
            dtype, sink = (BF16, F16)[(di + holes) % 2], bool((di + holes) % 2)
            # (the attention kernel walks 64-key tiles; no length above the caller's bound of 1000)
            case, _ = decode_case(dims, heads, page, 1, dtype, sink, seed=70 + di, holes=holes,
                                  lens=None if holes else (1, 63, 64, 65, 127, 128, 129, 0, 1000, 100, 513))
            form = ("plain", "slices", "hint")[(di + holes) % 3]
            env = dict(golden, MOJO_HIP_MLA_PREFILL_BYTES=str(one_seq)) if form == "slices" else golden
            kw = dict(max_total_seq_len=1000) if form != "plain" else {}
            out.append((form, case, env, kw))
    return out


@pytest.mark.parametrize("form,case,env,kw", golden_route_cases(), ids=ident)
def test_golden_rounding_decode_route(form, case, env, kw):
    run("golden-rounding decode", case, env, "mla_prefill_attn", **kw)


# ---- what the file as a whole must have seen --------------------------------------------------------------------------------
def planned():
    tags = {tag for _, _, tag in r512_cases() + general_cases() + absorbed_prefill_cases()} | {tag for _, _, tag, _ in window_cases()}
    return tags | {"mla_prefill_attn"}


def test_every_tag_was_seen_and_the_worst_deviations():
    """Runs last in the file: the launch tags the cases above left and, per route, the worst deviation they met."""
    for route, (ulp, rope, nope) in sorted(WORST.items()):
        print(f"{route}: map worst {ulp:.0f} ulp, selector worst |err| rope-coded {rope:.3e} nope-coded {nope:.3e}")
    print("launch tags seen:\n  " + "\n  ".join(sorted(SEEN)))
    want = planned()
    for kernel in ("ps", "oct"):                          # every split count of the issue on both r = 512 kernels
        assert {f"mla512:{kernel}:splits{n}" for n in (1, 2, 4, 5)} <= want
    assert {f"mla_latent:r{r}:splits{n}" for r in GENERAL for n in (1, 3, 6)} <= want
    if len(WORST) >= 8:                                   # (the whole file ran, not a selection of it)
        assert want == SEEN, sorted(want ^ SEEN)
