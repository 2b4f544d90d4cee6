"""GPU parity of the matrix-core paged decode's tile ring (csrc/paged_decode_mfma.h): the page-id windows, the counted
steady-state loop and its tail, in every form of the launch.

Conventions of tests/test_hip_decode_gqa.py: `make_decode_inputs`, the torch golden as the oracle, atol = rtol = 2e-2 (the
reference's own bound for this op).  Every case also asserts that a second call returns the same bits, that relabelling
the pages (permuted pools, remapped table) changes no bit, and that the launch took the form the case is about.

Shapes are the smallest at which the ring can go wrong: a wave's chunk of 1 .. 8 tiles and more (the loop runs from five
tiles on, the tail covers the last one to four), short last chunks, chunks with one and with two id-window hand-overs (windows
start 60 sub-tiles apart; the second hand-over installs a window that was requested inside the loop), the window jump of a
sliding-window row, holes at the window seams and behind a hand-over, and table entries the kernel must never turn into an address.
"""
import functools

import pytest
import torch

import oracle.swa
from hip_utils import DEV, assert_close_tree, hip_cls, last_launch, switch_env, to_cpu, torch_cls
from test_hip_decode_gqa import make_decode_inputs

pytestmark = pytest.mark.gpu
ATOL = RTOL = 2e-2

RING_LENS = [1, 15, 16, 17, 32, 33, 48, 49, 64, 65, 80, 81, 96, 97, 112, 113, 128, 129, 257, 401]
RING_LENS_D64 = [1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 159, 160, 161, 192, 193, 257, 401]   # 32-token steps
FORMS = {"default": ({}, "decode_mfma:paired"), "no_pair": ({"MOJO_HIP_DECODE_PAIR": "0"}, "decode_mfma:fused"),
         "no_fuse": ({"MOJO_HIP_DECODE_FUSE": "0"}, "decode_mfma:split+merge")}


def relabel(k, v, table, seed=3):
    """The same cache with its physical pages renumbered: new page p holds old page perm[p]."""
    g = torch.Generator().manual_seed(seed)
    perm = torch.randperm(k.shape[0], generator=g)
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(perm.numel())
    return k[perm], v[perm], torch.where(table >= 0, inv[table.clamp(min=0).long()].to(torch.int32), table)


def run_checked(op, inputs, want, form, **kw):
    """One case on the GPU: the form, the oracle, launch-to-launch determinism, page relabelling.  Returns the output."""
    q, k, v, lens, table = inputs
    dev = [t.to(DEV) for t in inputs]
    got = op(*dev, **kw)
    torch.cuda.synchronize()
    name = last_launch()
    assert name.startswith(form[0]) and name.endswith(form[1]), (name, form)
    if want is not None:
        assert_close_tree(to_cpu(got), want, ATOL, RTOL)
    assert torch.equal(op(*dev, **kw), got)
    k2, v2, table2 = relabel(k, v, table)
    assert torch.equal(op(dev[0], k2.to(DEV), v2.to(DEV), dev[3], table2.to(DEV), **kw), got)
    return got


@functools.lru_cache(maxsize=None)
def ring_case(d, dtype):
    lens = RING_LENS if d == 128 else RING_LENS_D64
    inputs = make_decode_inputs(len(lens), 8, 2, d, 0, 16, dtype=dtype, lens=lens, seed=d + 5)
    return inputs, torch_cls("MojoPagedDecodeGQA")()(*inputs)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("d,dtype", [(128, torch.bfloat16), (64, torch.bfloat16), (128, torch.float16)], ids=["d128", "d64", "fp16"])
def test_ring_phases(d, dtype, form):
    """One row per length: chunks of one to eight tiles (and of 4 to 26 in the unpaired forms' longest rows), full and partial
    last tiles, last chunks of a single tile."""
    env, want_form = FORMS[form]
    inputs, want = ring_case(d, dtype)
    with switch_env(**env):
        run_checked(hip_cls("MojoPagedDecodeGQA")(), inputs, want, (want_form, ""))


LONG_LENS = [5000, 2100, 1025]
HANDOVER_LENS = [6144, 2100, 1025]          # row 0: three chunks of 2 048 tokens = 128 sub-tiles, two window hand-overs per wave
LONG_CHUNK = 2048


def seq_chunk(n, n_chunks, cap=LONG_CHUNK):
    """Tokens of one wave's chunk of a row of n tokens (the kernel's per-sequence rule: equal pieces, whole tiles, >= 128)."""
    c = max(-(-n // n_chunks), 128)
    return min(-(-c // 16) * 16, cap)


@functools.lru_cache(maxsize=None)
def long_case(hq, page, lens=tuple(LONG_LENS)):
    return make_decode_inputs(len(lens), hq, 1, 128, 0, page, lens=list(lens), seed=hq + page)


@pytest.mark.parametrize("hq,page", [(4, 16), (4, 64), (8, 16)], ids=["G4_page16", "G4_page64", "G8_page16"])
def test_long_chunks_cross_id_windows(hq, page):
    """Three chunks per row of up to 1 680 tokens: a wave walks 105 sub-tiles, i.e. hands its id window over once (at sub-tile
    60, to the second window of the prologue); at page 64 four sub-tiles share a table entry."""
    inputs = long_case(hq, page)
    want = torch_cls("MojoPagedDecodeGQA")()(*inputs)
    with switch_env(MOJO_HIP_DECODE_CHUNK=str(LONG_CHUNK)):
        run_checked(hip_cls("MojoPagedDecodeGQA")(), inputs, want, ("decode_mfma:fused", ""))


@pytest.mark.parametrize("hq,page,d", [(4, 16, 128), (4, 64, 128), (8, 16, 128), (4, 16, 64)],
                         ids=["G4_page16", "G4_page64", "G8_page16", "G4_d64"])
def test_windows_refilled_inside_the_loop_are_used(hq, page, d):
    """A 6 144-token row in three chunks of 2 048 tokens: every wave walks 128 sub-tiles and hands its id window over twice,
    at sub-tiles 60 and 120.  The window it reads from sub-tile 120 on was requested inside the loop, at the first hand-over
    (both windows of the 105-sub-tile case above come from the prologue): a wrong base or a missing wait there is a wrong
    page, which the oracle and the page relabelling see.  Also at head_dim 64 (two sub-tiles per step)."""
    assert seq_chunk(HANDOVER_LENS[0], 3) // 16 == 128
    inputs = make_decode_inputs(len(HANDOVER_LENS), hq, 1, d, 0, page, lens=HANDOVER_LENS, seed=hq + page + d)
    want = torch_cls("MojoPagedDecodeGQA")()(*inputs)
    with switch_env(MOJO_HIP_DECODE_CHUNK=str(LONG_CHUNK)):
        run_checked(hip_cls("MojoPagedDecodeGQA")(), inputs, want, ("decode_mfma:fused", ""))


def hole_positions():
    """{name: (row lengths, page of row 0 that becomes -1)}.  The issue's positions on the 5 000-token row (chunks of 105
    pages), and on the 6 144-token row (chunks of 128 pages) the seam of two id windows — windows start 60 sub-tiles apart,
    lanes 60-63 of one repeat lanes 0-3 of the next — and the page just behind the second hand-over."""
    first = seq_chunk(LONG_LENS[0], 3) // 16                      # first page of the second wave's chunk
    out = {"chunk_first": (LONG_LENS, first), "chunk_63": (LONG_LENS, first + 63), "chunk_64": (LONG_LENS, first + 64),
           "chunk_65": (LONG_LENS, first + 65), "row_last": (LONG_LENS, (LONG_LENS[0] + 15) // 16 - 1)}
    first = seq_chunk(HANDOVER_LENS[0], 3) // 16
    for k in (59, 60, 61, 119, 120, 121):
        out[f"seam_{k}"] = (HANDOVER_LENS, first + k)
    return out


@pytest.mark.parametrize("where", list(hole_positions()))
def test_holes_at_the_window_seams(where):
    """One -1 in row 0's table: everything behind it reads as zero K/V (the golden's `break`), in the wave that owns the hole
    and in every wave behind it — at the first page of a chunk, at pages 63 - 65 of a chunk, at the row's last page, around
    the seam of two id windows (sub-tiles 59 - 61) and around the second hand-over (119 - 121)."""
    lens, page = hole_positions()[where]
    q, k, v, lens_t, table = long_case(4, 16, tuple(lens))
    table = table.clone()
    table[0, page] = -1
    inputs = (q, k, v, lens_t, table)
    want = torch_cls("MojoPagedDecodeGQA")()(*inputs)
    with switch_env(MOJO_HIP_DECODE_CHUNK=str(LONG_CHUNK)):
        run_checked(hip_cls("MojoPagedDecodeGQA")(), inputs, want, ("decode_mfma:fused", ""))


def poisoned(lens, hq, hkv, extra_cols, used_pages, seed):
    """Inputs whose table is wider than any row needs: (inputs with the entries past each row's `used_pages` pointing at a
    valid page of NaN keys and values, the same with those entries -1).  Every id stays inside the pool."""
    q, k, v, lens_t, table = make_decode_inputs(len(lens), hq, hkv, 128, 0, 16, lens=lens, seed=seed)
    spare = sorted(set(range(k.shape[0])) - set(table[table >= 0].tolist()))
    poison = spare[0]
    k, v = k.clone(), v.clone()
    k[poison] = float("nan")
    v[poison] = float("nan")
    wide = torch.full((len(lens), table.shape[1] + extra_cols), -1, dtype=torch.int32)
    wide[:, : table.shape[1]] = table
    bad = wide.clone()
    for b, n in enumerate(used_pages):
        wide[b, n:] = -1
        bad[b, n:] = poison
    return (q, k, v, lens_t, bad), (q, k, v, lens_t, wide)


def test_entries_past_a_rows_pages_are_never_used():
    lens = [401, 129, 16, 1, 700, 1025]
    bad, clean = poisoned(lens, 8, 2, 9, [(n + 15) // 16 for n in lens], seed=21)
    op = hip_cls("MojoPagedDecodeGQA")()
    want = torch_cls("MojoPagedDecodeGQA")()(*clean)
    got = run_checked(op, bad, want, ("decode_mfma:", ""))
    assert torch.isfinite(got.float()).all()
    assert torch.equal(op(*[t.to(DEV) for t in clean]), got)


def test_entries_past_the_hint_are_never_used():
    """`max_total_seq_len` = 1 024 on 4 rows x 2 kv heads: eight chunks of 128 tokens, a capacity of exactly 64 pages.  Rows
    above it are truncated there, and the poison sits in column 64 — the page right behind the last one the launch may walk."""
    lens, hint = [1500, 1100, 1024, 700], 1024
    bad, clean = poisoned(lens, 8, 2, 3, [min((n + 15) // 16, hint // 16) for n in lens], seed=22)
    op = hip_cls("MojoPagedDecodeGQA")()
    want = torch_cls("MojoPagedDecodeGQA")()(clean[0], clean[1], clean[2], clean[3].clamp(max=hint), clean[4])
    got = run_checked(op, bad, want, ("decode_mfma:fused", ""), max_total_seq_len=hint)
    assert torch.isfinite(got.float()).all()
    assert torch.equal(op(*[t.to(DEV) for t in clean], max_total_seq_len=hint), got)


def paired_lens(kind):
    if kind == "pairs":                       # by length rank: (600, 0), (599, 1), then thirty pairs of equals
        return [600, 599] + [300] * 60 + [1, 0]
    g = torch.Generator().manual_seed(64)
    return torch.randint(0, 601, (64,), generator=g).tolist()


@pytest.mark.parametrize("kind", ["pairs", "ragged"])
def test_paired_form(kind):
    """B 64, 32 q / 8 kv heads, contexts <= 600: eight waves dealt between the two rows of a pair — seven and one for
    (long, 0) and (long, 1), four and four for equals."""
    lens = paired_lens(kind)
    inputs = make_decode_inputs(64, 32, 8, 128, 0, 16, lens=lens, seed=9)
    want = torch_cls("MojoPagedDecodeGQA")()(*inputs)
    got = run_checked(hip_cls("MojoPagedDecodeGQA")(), inputs, want, ("decode_mfma:paired", ""), max_total_seq_len=600)
    empty = [b for b, n in enumerate(lens) if n == 0]
    assert torch.count_nonzero(got[empty]) == 0


def test_grouped_form():
    """B 3, 64 q / 8 kv heads, ctx 5 000: rows of one chunk, of a few chunks and of many (several workgroups per row)."""
    lens = [100, 700, 5000]
    inputs = make_decode_inputs(3, 64, 8, 128, 0, 16, lens=lens, seed=7)
    want = torch_cls("MojoPagedDecodeGQA")()(*inputs)
    run_checked(hip_cls("MojoPagedDecodeGQA")(), inputs, want, ("decode_mfma:grouped+merge", ""), max_total_seq_len=5000)


@pytest.mark.parametrize("lens,glob,local", [([3000, 600, 100], 40, 500), ([520, 17, 40], 40, 500)], ids=["gap", "collapsed"])
def test_sliding_window_jump_inside_an_id_window(lens, glob, local):
    """len 3 000, global 40, local 500: the walk jumps from token 48 to token 2 496, three sub-tiles into the first id window.
    len 520: the local range starts inside the global one and the two collapse into one walk without a jump."""
    kw = dict(gqa_layout="AABB", global_window_size=glob, local_window_size=local)
    inputs = make_decode_inputs(len(lens), 8, 2, 128, 0, 16, lens=lens, seed=31)
    want = oracle.swa.TorchPagedDecodeSWA(**kw).forward(*inputs)
    run_checked(hip_cls("MojoPagedDecodeSWA")(**kw), inputs, want, ("decode_mfma:", ":swa"))
