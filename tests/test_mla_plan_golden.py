"""The launch plan of the MLA latent attention, pinned without a GPU: what `mojo_hip_mla_latent_attn_workspace_bytes` answers
over the grid of scripts/make_mla_plan_golden.py, against tests/golden/mla_plan_bytes.json.

The file was recorded from a library built at the commit before `mla_plan` replaced the sizing arithmetic that the query and
the entry point each had (scripts/make_mla_plan_golden.py says how to record it again): every digest and every sampled size
must be what that library answered, under each MOJO_HIP_MLA_SPLITS the grid is walked with.  Two identities hold on the whole
grid besides."""
import importlib.util
import json
import os

import pytest

from conftest import ROOT
from visibility_mla import default_splits

_spec = importlib.util.spec_from_file_location("make_mla_plan_golden", os.path.join(ROOT, "scripts", "make_mla_plan_golden.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

with open(G.FIXTURE) as _f:
    RECORDED = json.load(_f)


@pytest.fixture(scope="module")
def lib():
    from mojo_opset_amd.backends.hip import lib as L

    return L.load()


@pytest.mark.parametrize("env", list(G.ENVS))
def test_query_answers_what_was_recorded(lib, env):
    with G.plan_env(env):
        got = G.answers(lib)
    assert RECORDED["sample_stride"] == G.SAMPLE_STRIDE
    want = RECORDED["samples"][env]
    mine = list(got[::G.SAMPLE_STRIDE])
    if mine != want:                                      # name the first sampled case that moved
        cases = list(G.walk())[::G.SAMPLE_STRIDE]
        i = next(i for i, (a, b) in enumerate(zip(mine, want)) if a != b) if len(mine) == len(want) else 0
        pytest.fail(f"{env} / {cases[i]}: {mine[i]} B, recorded {want[i]} B")
    assert G.digest(got) == RECORDED["digest"][env], f"{env}: a size outside the samples moved"


def test_environments_steer_the_plan():
    """(the walk is not vacuous: each split count gives sizes of its own)"""
    assert len(set(RECORDED["digest"].values())) == len(G.ENVS)


@pytest.mark.parametrize("env", list(G.ENVS))
def test_answer_is_whole_slots(lib, env):
    """Beyond the 64 bytes of slack the workspace is a whole number of (r + 2) * 4-byte slots per (token, head): the fp32 partial
    of one split and its (maximum, sum) pair.  Under the default environment that number is the split count the heuristic
    gives — `default_splits`, which the visibility test builds its tile edges from — and a single split needs no slot."""
    forced = int(G.ENVS[env].get("MOJO_HIP_MLA_SPLITS", 0))
    seen = set()
    with G.plan_env(env):
        got = G.answers(lib)
    for (tokens, heads, r, max_len), size in zip(G.walk(), got):
        want = forced or default_splits(tokens, heads, r, 64 if r == 512 else 32, max_len)
        if size <= 64:
            assert size == 64 and (want == 1 or tokens == 0), (tokens, heads, r, max_len)
            continue
        per_row, rest = divmod(size - 64, (r + 2) * 4)
        assert rest == 0 and per_row % (tokens * heads) == 0, (tokens, heads, r, max_len)
        assert per_row // (tokens * heads) == want, (tokens, heads, r, max_len)
        seen.add(want)
    if env == "default":                                  # both caps of the heuristic and the values between
        assert {2, 4, 64} <= seen and any(n not in (2, 4, 64) for n in seen)
