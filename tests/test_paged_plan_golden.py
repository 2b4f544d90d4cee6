"""The launch plans of the paged attention family, pinned without a GPU: what the six `*_workspace_bytes` queries answer over
the grid of scripts/make_paged_plan_golden.py, against tests/golden/paged_plan_bytes.json.

The file was recorded from a library built at the commit before `decode_plan` / `prefill_plan` replaced the copied sizing
arithmetic (scripts/make_paged_plan_golden.py says how to record it again): every digest and every sampled size must be what
that library answered, under each of the environments that steer the plans.  Two identities hold on the whole grid besides."""
import collections
import importlib.util
import json
import os

import pytest

from conftest import ROOT

_spec = importlib.util.spec_from_file_location("make_paged_plan_golden", os.path.join(ROOT, "scripts", "make_paged_plan_golden.py"))
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


def test_environments_steer_the_plans(lib):
    """(the walk is not vacuous: each environment moves the sizes of the family it belongs to, and of no other)"""
    d = RECORDED["digest"]
    for env in ("chunk256", "grouped0", "fuse0", "mfma0", "mfma1"):
        assert d[env]["decode_gqa"] != d["default"]["decode_gqa"], env
        assert all(d[env][q] == d["default"][q] for q in ("prefill_gqa", "prefill_swa", "prefill_kv8")), env
    assert d["chunk256"]["decode_kv8"] != d["default"]["decode_kv8"]
    assert all(d[env]["decode_kv8"] == d["default"]["decode_kv8"] for env in ("grouped0", "fuse0", "mfma0", "mfma1"))
    for env in ("ksplit1", "ksplit3"):
        assert all(d[env][q] != d["default"][q] for q in ("prefill_gqa", "prefill_swa", "prefill_kv8")), env
        assert all(d[env][q] == d["default"][q] for q in ("decode_gqa", "decode_swa", "decode_kv8")), env


def test_grid_crosses_the_branches_of_the_plans(lib):
    """Chunk counts of 1, 4, exactly 8 and more; key splits on both sides of 256 blocks and of 1024 keys; zeros."""
    chunks = set()
    for (batch, hq, hkv, dim, page, width, hint), size in zip(G.walk("decode_gqa"), G.answers(lib, "decode_gqa")):
        if min(batch, hq, hkv) <= 0:
            assert size == 0
        elif hq >= hkv:
            slots, rest = divmod(size - 256, (dim + 2) * 4)
            assert rest == 0 and slots % (batch * hkv * (hq // hkv)) == 0
            chunks.add(slots // (batch * hkv * (hq // hkv)))
    assert {1, 4, 8} <= chunks and max(chunks) > 8
    seen = collections.Counter()
    for (tokens, batch, hq, hkv, dim, page, width, hint_q, hint_kv), size in zip(G.walk("prefill_gqa"), G.answers(lib, "prefill_gqa")):
        if min(tokens, batch, hq, hkv) <= 0 or hq % hkv:
            assert size == 0
            continue
        max_q = hint_q if 0 < hint_q < tokens else tokens
        blocks = -(-max_q // (128 // (hq // hkv))) * hkv * batch
        cap = hint_kv if 0 < hint_kv < page * width else page * width
        seen[(blocks <= 256, cap >= 1024, size > 0)] += 1
    assert all(seen[k] > 0 for k in ((True, True, True), (True, False, False), (False, True, False), (False, False, False)))
    assert seen[(True, False, True)] == seen[(False, True, True)] == seen[(False, False, True)] == 0


@pytest.mark.parametrize("env", ["default", "fuse0", "ksplit3"])
def test_no_window_is_the_gqa_query(lib, env):
    none = G.WINDOWS.index((-1, 0))
    with G.plan_env(env):
        for kind in ("decode", "prefill"):
            assert G.answers(lib, kind + "_swa")[none::len(G.WINDOWS)] == G.answers(lib, kind + "_gqa"), kind


@pytest.mark.parametrize("env", ["default", "ksplit1", "ksplit3"])
def test_kv8_prefill_holds_the_16bit_prefill_of_its_scratch(lib, env):
    """The int8 prefill runs the 16-bit one over ppb scratch pages per sequence (ceil of the hinted capacity over the page, at
    least one): its workspace holds at least what that launch asks for."""
    with G.plan_env(env):
        for args, size in zip(G.walk("prefill_kv8"), G.answers(lib, "prefill_kv8")):
            tokens, batch, hq, hkv, dim, page, width, hint_q, hint_kv = args
            cap = hint_kv if 0 < hint_kv < page * width else page * width
            ppb = max(-(-cap // page), 1)
            inner = lib.mojo_hip_paged_prefill_gqa_workspace_bytes(tokens, batch, hq, hkv, dim, page, ppb, hint_q, hint_kv)
            assert size >= inner, args
            assert size > 0 or min(tokens, batch, hq, hkv) <= 0 or hq % hkv
