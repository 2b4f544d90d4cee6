"""The visible key set of the linear prefill launches (`MojoSWA`), key by key (DESIGN §4.17 on the packed layout, §4.18).

The MAP and SELECTOR families of tests/visibility.py on contiguous K/V (tests/visibility_packed.py): the expectation is the
definition (`oracle.paged.window_mask`), exactly (map: 0 for an invisible key, ``storage(1 / n)`` within 1 ulp for a visible
one) or within the selector's 4 ulp at 1.0.  Sequences are adjacent in memory, so the keys a row must not see are its
neighbours' (one leaked key changes the integer row sum) and the poisoned unused tokens at both ends of the tensor.

The selector's targets are every row's own causal and window edges and both sides of every multiple of 16 (the keys a wave
stages) and 64 (the key tile, PF_KEYS), counted from the sequence's start AND from the tensor's start: with 5 leading tokens no
sequence starts on a multiple of either, so the two counts differ everywhere.

Every case forces its form — unsplit or four key slices, fast or general staging —, asserts the launch tag, and makes every
call twice (same bits)."""
import pytest
import torch

import visibility as V
import visibility_packed as VP
from hip_utils import DEV, hip_cls, switch_env

pytestmark = pytest.mark.gpu
BF16, F16 = torch.bfloat16, torch.float16
STRIDES = (16, 64)
# (Hq, Hkv, D, layout, dtype): G 1 2 4 8
GEOMS = [(4, 4, 64, "ABAB", BF16), (4, 2, 128, "AABB", F16), (8, 2, 96, "ABAB", BF16), (8, 1, 128, "AABB", F16)]
# (MOJO_HIP_PREFILL_KSPLIT, MOJO_HIP_PREFILL_FAST_STAGE)
STAGINGS = [(1, 1), (4, 1), (1, 0), (4, 0)]
# (glob, local, dtype): the type in which the row sum of every row resolves n +- 1 (tests/test_hip_visibility.py WINDOWS)
WINDOWS = [(None, 0, BF16), (1, 1, BF16), (4, 15, BF16), (16, 16, F16), (17, 17, BF16), (4, 63, BF16), (16, 64, F16),
           (17, 65, BF16), (None, 127, F16), (1, 127, F16), (16, None, BF16), (100, 63, F16), (4, 2000, F16)]


def lens(group, windowed):
    """(kv_lens, q_lens): a query block (128 // G rows) less one row, whole, plus one row, and one row; a cached prefix of 0, of
    one key, one that ends inside a 64-key tile; 16 key tiles (the length a split launch cuts); an empty sequence.  With a
    window: a cached prefix long enough for a gap of several whole tiles."""
    qb = 128 // group
    kv = [qb - 1, qb + 1, qb + 1 + 37, 300, 1024, 0]
    q = [qb - 1, qb, qb + 1, 1, 40, 0]
    if windowed:
        kv.append(900)
        q.append(qb + 3)
    return kv, q


class Tagged:
    """``op`` with every call checked against the launch tag it must leave."""

    def __init__(self, op, want):
        self.op, self.want = op, want

    def forward(self, *args, **kw):
        from mojo_opset_amd.backends.hip import lib

        lib.launch_history(clear=True)
        out = self.op.forward(*args, **kw)
        torch.cuda.synchronize()
        got = lib.launch_history()
        assert got == self.want, (got, self.want)
        return out


def cases():
    out = []
    for gi, (hq, hkv, d, layout, dtype) in enumerate(GEOMS):
        for k in range(2):
            kv, q = lens(hq // hkv, False)
            case = VP.packed_case(kv, q, hq=hq, hkv=hkv, d=d, layout=layout, dtype=dtype, pad_tokens=3, seed=gi * 2 + k)
            out.append((case, STAGINGS[(gi + 2 * k + k * (gi % 2)) % 4]))
    for wi, (glob, local, dtype) in enumerate(WINDOWS):
        hq, hkv, d, layout, _ = GEOMS[wi % 4]
        kv, q = lens(hq // hkv, True)
        case = VP.packed_case(kv, q, hq=hq, hkv=hkv, d=d, layout=layout, dtype=dtype, glob=glob, local=local, pad_tokens=3,
                              seed=20 + wi)
        out.append((case, STAGINGS[(wi + wi // 4) % 4]))
    return out


def ident(v):
    if isinstance(v, V.Case):
        return f"{str(v.dtype)[6:]}-{v.hq}x{v.hkv}x{v.d}-{v.layout}-g{v.glob}-l{v.local}"
    if isinstance(v, tuple):
        return f"ksplit{v[0]}-fast{v[1]}"
    return None


def test_the_cases_cover_every_form():
    forms = {(staging, case.glob is not None or case.local is not None) for case, staging in cases()}
    assert forms == {(s, w) for s in STAGINGS for w in (False, True)}


@pytest.mark.parametrize("case,staging", cases(), ids=ident)
def test_linear_prefill(case, staging):
    ksplit, fast = staging
    swa = case.glob is not None or case.local is not None
    want = f"prefill_linear:default:{'fast' if fast else 'general'}_stage:ksplit{ksplit}{':swa' if swa else ''}"
    with switch_env(MOJO_HIP_PREFILL_KSPLIT=str(ksplit), MOJO_HIP_PREFILL_FAST_STAGE=str(fast)):
        op = Tagged(case.make(hip_cls(case.op)), want)
        for family in (V.MAP, V.SELECTOR):
            failures, err = VP.run_packed_family(case, family, op, device=DEV, strides=STRIDES, repeat=True)
            print(f"{case.op} {family}: worst {err:.3g} {'ulp' if family == V.MAP else 'abs'}  [{want}]")
            assert not failures, f"{family} {staging} {case}\n" + V.report(failures)
    # padding rows behind the last sequence are zeros (the comparer checked them: `V.unpack` returns them as one more entry)
