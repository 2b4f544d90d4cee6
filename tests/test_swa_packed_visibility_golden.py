"""tests/visibility_packed.py against the torch golden of `MojoSWA`, without a GPU: the map and the selector read back exactly
the keys the definition (`oracle.paged.window_mask`) makes visible, so what tests/test_hip_swa_packed_visibility.py demands of
the kernels is what the golden does."""
import pytest
import torch

import swa_packed_golden
import visibility as V
import visibility_packed as VP

CASES = [
    VP.packed_case([31, 33, 70, 300, 0], [31, 32, 33, 1, 0], hq=8, hkv=2, d=64, layout="ABAB", pad_tokens=3, seed=1),
    VP.packed_case([63, 65, 102, 300, 0, 400], [63, 64, 65, 1, 0, 67], hq=4, hkv=2, d=128, layout="AABB", dtype=torch.float16,
                   glob=4, local=63, pad_tokens=2, seed=2),
    VP.packed_case([40, 200], [40, 9], hq=2, hkv=2, d=64, glob=17, local=None, lead=0, tail=0, seed=3),
]


@pytest.mark.parametrize("family", [V.MAP, V.SELECTOR])
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c.hq}x{c.hkv}x{c.d}-g{c.glob}-l{c.local}")
def test_golden_attends_exactly_the_visible_keys(case, family):
    op = case.make(swa_packed_golden.TorchSWA)
    failures, _ = VP.run_packed_family(case, family, op, strides=(16, 64))
    assert not failures, V.report(failures)


def test_edge_targets_count_from_the_sequence_and_from_the_tensor():
    case = VP.packed_case([200, 100], [200, 100], hq=2, hkv=2, d=64, lead=5, tail=0)
    first = VP._edge_candidates(case, 0, (16, 64), 5)
    assert {15, 16, 63, 64} <= set(first)                        # from the sequence's start
    assert {10, 11, 58, 59, 122, 123} <= set(first)              # 5 + t on a multiple of 16 / 64
    second = VP._edge_candidates(case, 1, (64,), 205)
    assert set(second) == {63, 64, 50, 51}                       # 205 + 51 = 256
    plan = VP.packed_selector_plan(case, (16, 64))
    met = {int(t) for _, targets in plan for t in targets[0].flatten()}
    assert set(first) <= met


def test_a_leaked_neighbour_key_is_seen_by_the_map():
    """An operator that reads one key past a sequence's end (its neighbour's first) fails the map."""
    case = CASES[0]

    golden = case.make(swa_packed_golden.TorchSWA)

    class Leaky:
        @staticmethod
        def forward(q, k, v, cu_q, cu_kv, **kw):
            cu_kv = cu_kv.clone()
            cu_kv[1] += 1                                        # sequence 0 ends one key late ... in its neighbour
            return golden.forward(q, k, v, cu_q, cu_kv, **kw)
    failures, _ = VP.run_packed_family(case, V.MAP, Leaky)
    assert failures and failures[0][0] == 0
