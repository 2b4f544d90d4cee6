"""The planners of the 8-bit GEMM entry points, pinned without a GPU: what `mojo_hip_quant_gemm_workspace_bytes` and
`mojo_hip_group_quant_gemm_workspace_bytes` answer over the grid of scripts/make_quant_plan_golden.py, against
tests/golden/quant_plan_bytes.json.

The file was recorded from a library built at the commit before `plan_quant_gemm` / `plan_group_quant_gemm` and the
`*_max_splitk` bounds beside them replaced the route chains and the hand-kept maxima of the queries
(scripts/make_quant_plan_golden.py says how to record it again): every digest and every sampled size must be what that library
answered, oversizing included, under each of the environments that steer the split models.

Sizes: the dense query answers 64 + split * m * n * 4 bytes where some route may split and 64 where none does; the grouped one
its prefix arrays (what it answers for no rows) plus the same slabs.

Two departures from the grid the planners' issue named, both because of what the recorded library answers:
* K = 65536 and N = 192, 512 were added.  Up to K = 18432 the weight stream's own split never passes the 256 x 256 kernel's
  (32 slices from K = 8192 on), so MOJO_HIP_GEMM_WAVES moved no dense answer; at K = 65536 the stream reaches 64 slices and the
  waves show (65 x 65536 x 192: 64 slices, 42 with four waves forced).
* The dense walk has no m = 0: that library divides by the zero tiles of an empty product (SIGFPE where K has two K-tiles and
  N % 4 == 0) and so has nothing to record.  `quant_max_splitk` answers no split for no rows; the last test pins m = 0 to the
  64 bytes the recorded library answers where it answers at all (K = 64, 128)."""
import importlib.util
import json
import os

import pytest

from conftest import ROOT

_spec = importlib.util.spec_from_file_location("make_quant_plan_golden", os.path.join(ROOT, "scripts", "make_quant_plan_golden.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

with open(G.FIXTURE) as _f:
    RECORDED = json.load(_f)


@pytest.fixture(scope="module")
def lib():
    from mojo_opset_amd.backends.hip import lib as L

    return L.load()


@pytest.mark.parametrize("env", list(G.ENVS))
def test_queries_answer_what_was_recorded(lib, env):
    with G.plan_env(env):
        got = {q: G.answers(lib, q) for q in G.QUERIES}
    assert RECORDED["sample_stride"] == G.SAMPLE_STRIDE
    for q, values in got.items():
        want = RECORDED["samples"][env][q]
        mine = list(values[::G.SAMPLE_STRIDE])
        if mine != want:                                  # name the first sampled case that moved
            cases = list(G.walk(q))[::G.SAMPLE_STRIDE]
            i = next(i for i, (a, b) in enumerate(zip(mine, want)) if a != b) if len(mine) == len(want) else 0
            pytest.fail(f"{env} / {q}{cases[i]}: {mine[i]} B, recorded {want[i]} B")
        assert G.digest(values) == RECORDED["digest"][env][q], f"{env} / {q}: a size outside the samples moved"


def _dense_splits(lib):
    """The split behind every dense answer: (size - 64) / (4 m n), 1 where no slab is asked for."""
    out = {}
    for (m, k, n), size in zip(G.walk("quant_gemm"), G.answers(lib, "quant_gemm")):
        if size == 64:
            out[(m, k, n)] = 1
            continue
        split, rest = divmod(size - 64, 4 * m * n)
        assert rest == 0 and split > 1, (m, k, n, size)
        out[(m, k, n)] = split
    return out


def test_grid_crosses_the_split_models(lib):
    """(the walk is not vacuous: no split, the tiles' splits of 2..16, and the decode-sized splits above 16)"""
    with G.plan_env("default"):
        splits = _dense_splits(lib)
    seen = set(splits.values())
    assert 1 in seen and any(2 <= s <= 16 for s in seen) and max(seen) > 16, sorted(seen)
    assert splits[(1, 8192, 64)] >= 32                    # quant_splitk: one tile over 64 K-tiles


def test_environments_steer_the_plans():
    """Each forced split moves both queries; the waves per workgroup are the dense weight stream's alone."""
    d = RECORDED["digest"]
    for env in ("splitk1", "splitk3", "splitk40"):
        assert all(d[env][q] != d["default"][q] for q in G.QUERIES), env
        assert all(d[env][q] != d[other][q] for q in G.QUERIES for other in ("splitk1", "splitk3", "splitk40") if other != env), env
    for env in ("waves4", "waves7"):
        assert d[env]["quant_gemm"] != d["default"]["quant_gemm"], env
        assert d[env]["group_quant_gemm"] == d["default"]["group_quant_gemm"], env
    assert d["waves4"]["quant_gemm"] != d["waves7"]["quant_gemm"]


@pytest.mark.parametrize("env", list(G.ENVS))
def test_dense_query_holds_the_grouped_slabs_of_one_group(lib, env):
    """One group is a dense product: where both queries ask for slabs, the dense one (an upper bound over layouts and routes)
    asks for at least the grouped one's."""
    both = 0
    with G.plan_env(env):
        for m, k, n in G.walk("quant_gemm"):
            dense = lib.mojo_hip_quant_gemm_workspace_bytes(m, k, n) - 64
            grouped = lib.mojo_hip_group_quant_gemm_workspace_bytes(m, k, n, 1) - lib.mojo_hip_group_quant_gemm_workspace_bytes(0, k, n, 1)
            assert dense >= 0 and grouped >= 0 and dense % 4 == 0 and grouped % 4 == 0, (m, k, n)
            if dense > 0 and grouped > 0:
                both += 1
                assert dense >= grouped, (m, k, n, dense, grouped)
    assert both > 0 or env == "splitk1"


def test_no_rows_need_no_slabs(lib):
    for k in G.K:
        for n in G.N:
            assert lib.mojo_hip_quant_gemm_workspace_bytes(0, k, n) == 64, (k, n)
            assert lib.mojo_hip_group_quant_gemm_workspace_bytes(0, k, n, 1) == 80, (k, n)
