"""Write tests/golden/mla_plan_bytes.json: what `mojo_hip_mla_latent_attn_workspace_bytes` answers over a grid of geometries.

Usage: MOJO_HIP_LIB=/path/to/parent/libmojo_hip.so python scripts/make_mla_plan_golden.py

The query is pure host code (no GPU needed).  Record the file from a library built at the commit BEFORE a change of the launch
plan (`mla_plan`, `mla_splits` in csrc/mla_attn.hip), never from the code under test: tests/test_mla_plan_golden.py then pins
the changed plan to the recorded sizes.  The test imports the grid and the walk below, so both sides see the same cases.

Per environment the file holds a sha256 over every answer of the grid, in grid order, and the explicit answers of every
SAMPLE_STRIDE-th case (what a failing test can point at).
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

FIXTURE = os.path.join(ROOT, "tests", "golden", "mla_plan_bytes.json")
SAMPLE_STRIDE = 97                       # prime: the samples walk through every axis of the grid

# environments the grid is walked under: the heuristic, one split, a few, more than the heuristic ever takes
ENVS = {
    "default": {},
    "splits1": {"MOJO_HIP_MLA_SPLITS": "1"},
    "splits5": {"MOJO_HIP_MLA_SPLITS": "5"},
    "splits200": {"MOJO_HIP_MLA_SPLITS": "200"},
}
PLAN_SWITCHES = sorted({k for env in ENVS.values() for k in env})

# Every branch of `mla_splits` and of the head-block rule: no token, 256 / tiles on both sides of 1, 2, 4 and 64 (with one and
# two head blocks per token); one, a partial second and two blocks of 64 heads; the rank that counts head blocks and four that
# do not; capacities around the 256 keys a split holds at least, around 64 splits' worth (16384), and far beyond.
Q_TOKENS = (0, 1, 2, 3, 4, 5, 64, 128, 129, 255, 256, 257, 1024)
HEADS = (1, 16, 63, 64, 65, 72, 128)
RANKS = (32, 64, 128, 256, 512)
MAX_KV_LENS = (0, 1, 255, 256, 257, 1024, 4096, 16384, 16385, 65536, 1 << 20)


def walk():
    """(q_tokens, heads, kv_lora_rank, max_kv_len) in grid order."""
    return itertools.product(Q_TOKENS, HEADS, RANKS, MAX_KV_LENS)


def answers(lib):
    """array('q') of what the query answers over the grid, under the environment in effect."""
    fn = lib.mojo_hip_mla_latent_attn_workspace_bytes
    return array.array("q", (fn(*args) for args in walk()))


def digest(values):
    return hashlib.sha256(values.tobytes()).hexdigest()


class plan_env:
    """Walk the grid under one of ENVS: every switch the plan reads is set or unset, both layers re-read them."""

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
            got = answers(lib)
        out["digest"][env] = digest(got)
        out["samples"][env] = list(got[::SAMPLE_STRIDE])
    with open(FIXTURE, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print(FIXTURE, os.path.getsize(FIXTURE), "bytes;", len(got), "cases per environment")


if __name__ == "__main__":
    main()
