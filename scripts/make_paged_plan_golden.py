"""Write tests/golden/paged_plan_bytes.json: what the six paged-attention workspace queries answer over a grid of geometries.

Usage: MOJO_HIP_LIB=/path/to/parent/libmojo_hip.so python scripts/make_paged_plan_golden.py

The queries are pure host code (no GPU needed).  Record the file from a library built at the commit BEFORE a change of the
launch plans (`decode_plan`, `prefill_plan` and what they call), never from the code under test: tests/test_paged_plan_golden.py
then pins the changed plans to the recorded sizes.  The test imports the grid and the walk below, so both sides see the same cases.

Per (environment, query) the file holds a sha256 over every answer of the grid, in grid order, and the explicit answers of
every SAMPLE_STRIDE-th case (what a failing test can point at).
"""
import array
import hashlib
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIXTURE = os.path.join(ROOT, "tests", "golden", "paged_plan_bytes.json")
SAMPLE_STRIDE = 499                      # prime: the samples walk through every axis of the grid

# environments the grid is walked under (the switches the plans read)
ENVS = {
    "default": {},
    "chunk256": {"MOJO_HIP_DECODE_CHUNK": "256"},
    "grouped0": {"MOJO_HIP_DECODE_GROUPED": "0"},
    "fuse0": {"MOJO_HIP_DECODE_FUSE": "0"},
    "mfma0": {"MOJO_HIP_DECODE_MFMA": "0"},
    "mfma1": {"MOJO_HIP_DECODE_MFMA": "1"},
    "ksplit1": {"MOJO_HIP_PREFILL_KSPLIT": "1"},
    "ksplit3": {"MOJO_HIP_PREFILL_KSPLIT": "3"},
}
PLAN_SWITCHES = sorted({k for env in ENVS.values() for k in env})

# (q_heads, kv_heads): groups of 1, 2, 4, 5, 8 and 16; 12 / 8 does not divide; no heads at all
HEADS = [(8, 8), (8, 4), (32, 8), (40, 8), (64, 8), (8, 1), (16, 1), (12, 8), (0, 8), (8, 0)]
# (local, global) of the SWA queries: none, local only, global only, both, local = 0 without and with a global window
WINDOWS = [(-1, 0), (1023, 0), (-1, 64), (255, 4), (0, 0), (0, 16)]
HINTS = ("none", "below", "above")       # of a capacity `cap`: 0, cap // 2, 2 * cap


def _hint(kind, cap):
    return {"none": 0, "below": cap // 2, "above": 2 * cap}[kind]


def decode_cases():
    """(batch, q_heads, kv_heads, head_dim, page, max_pages, hint).  Pages: below 16, powers of two, not a power of two.
    Table widths from none to 64 K tokens: with the batches they give one chunk, 4, exactly 8 and more than 8 per row."""
    for batch, (hq, hkv), dim, page, width, hint in itertools.product(
            (0, 1, 2, 3, 8, 16, 64, 255, 256), HEADS, (64, 80, 96, 128), (8, 16, 48, 128), (0, 1, 16, 64, 256, 2048), HINTS):
        yield batch, hq, hkv, dim, page, width, _hint(hint, page * width)


def prefill_cases():
    """(total_tokens, batch, q_heads, kv_heads, head_dim, page, max_pages, max_q hint, max_kv hint).  Tokens x heads x batch
    put the block count on both sides of 256; pages x widths put the key capacity on both sides of 1024."""
    for tokens, batch, (hq, hkv), dim, page, width, hint_q, hint_kv in itertools.product(
            (0, 1, 300, 512, 2048, 40000), (0, 1, 2, 8), HEADS, (64, 128), (8, 16, 48), (0, 63, 64, 65, 256, 4096), (0, 100), HINTS):
        yield tokens, batch, hq, hkv, dim, page, width, hint_q, _hint(hint_kv, page * width)


# query name -> (C symbol, cases, trailing windows or None)
QUERIES = {
    "decode_gqa": ("mojo_hip_paged_decode_gqa_workspace_bytes", decode_cases, None),
    "decode_swa": ("mojo_hip_paged_decode_swa_workspace_bytes", decode_cases, WINDOWS),
    "decode_kv8": ("mojo_hip_paged_decode_gqa_kv8_workspace_bytes", decode_cases, None),
    "prefill_gqa": ("mojo_hip_paged_prefill_gqa_workspace_bytes", prefill_cases, None),
    "prefill_swa": ("mojo_hip_paged_prefill_swa_workspace_bytes", prefill_cases, WINDOWS),
    "prefill_kv8": ("mojo_hip_paged_prefill_gqa_kv8_workspace_bytes", prefill_cases, None),
}


def walk(query):
    """The argument tuples of ``query`` in grid order (the windowed queries: every case under every window)."""
    _, cases, windows = QUERIES[query]
    if windows is None:
        return cases()
    return (case + win for case in cases() for win in windows)


def answers(lib, query):
    """array('q') of what ``query`` answers over its grid, under the environment in effect."""
    fn = getattr(lib, QUERIES[query][0])
    return array.array("q", (fn(*args) for args in walk(query)))


def digest(values):
    return hashlib.sha256(values.tobytes()).hexdigest()


class plan_env:
    """Walk the grid under one of ENVS: every switch the plans read is set or unset, both layers re-read them."""

    def __init__(self, name):
        self.values = ENVS[name]

    def __enter__(self):
        from mojo_opset_amd import switches

        self.old = {k: os.environ.pop(k, None) for k in PLAN_SWITCHES}
        os.environ.update(self.values)
        switches.reload()

    def __exit__(self, *exc):
        from mojo_opset_amd import switches

        for k, v in self.old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
        switches.reload()
        return False


def main():
    from mojo_opset_amd.backends.hip import lib as L

    lib = L.load()
    out = {"library": lib.mojo_hip_version().decode(), "sample_stride": SAMPLE_STRIDE, "digest": {}, "samples": {}}
    for env in ENVS:
        with plan_env(env):
            got = {q: answers(lib, q) for q in QUERIES}
        out["digest"][env] = {q: digest(v) for q, v in got.items()}
        out["samples"][env] = {q: list(v[::SAMPLE_STRIDE]) for q, v in got.items()}
    with open(FIXTURE, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print(FIXTURE, os.path.getsize(FIXTURE), "bytes;", {q: len(v) for q, v in got.items()}, "cases per environment")


if __name__ == "__main__":
    main()
