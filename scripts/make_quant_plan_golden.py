"""Write tests/golden/quant_plan_bytes.json: what the two 8-bit GEMM workspace queries answer over a grid of shapes.

Usage: MOJO_HIP_LIB=/path/to/parent/libmojo_hip.so MOJO_HIP_ALLOW_STALE=1 python scripts/make_quant_plan_golden.py

The queries are pure host code (no GPU needed).  Record the file from a library built at the commit BEFORE a change of the
planners (`plan_quant_gemm`, `plan_group_quant_gemm`, `quant_max_splitk` and the models they ask), never from the code under
test: tests/test_quant_plan_golden.py then pins the changed planners to the recorded sizes, oversizing included.  The test
imports the grid and the walk below, so both sides see the same cases.

Per (environment, query) the file holds a sha256 over every answer of the grid, in grid order, and the explicit answers of
every SAMPLE_STRIDE-th case (what a failing test can point at).  Digest and environment context follow
scripts/make_paged_plan_golden.py.
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

FIXTURE = os.path.join(ROOT, "tests", "golden", "quant_plan_bytes.json")
SAMPLE_STRIDE = 37                       # prime: the samples walk through every axis of the grid

# environments the grid is walked under (the switches the split models read)
ENVS = {
    "default": {},
    "splitk1": {"MOJO_HIP_GEMM_SPLITK": "1"},
    "splitk3": {"MOJO_HIP_GEMM_SPLITK": "3"},
    "splitk40": {"MOJO_HIP_GEMM_SPLITK": "40"},         # past every clamp of the unforced models: taken as it is
    "waves4": {"MOJO_HIP_GEMM_WAVES": "4"},
    "waves7": {"MOJO_HIP_GEMM_WAVES": "7"},
}
PLAN_SWITCHES = sorted({k for env in ENVS.values() for k in env})

# rows: none, the GEMV's 1..4, both sides of the weight stream's 16 / 32 / 64 / 128-row forms, of one and two 128- and 256-row tiles
M = (0, 1, 4, 5, 16, 17, 32, 64, 65, 100, 128, 129, 200, 256, 512, 1024, 4096)
# K: below one K-tile, one and two K-tiles, a K-tile that is no 256-byte block, the models' long K; 65536: the only K here at which
# the weight stream's own split (at most a quarter of the 256-byte K blocks) passes the 256 x 256 kernel's 32 slices, so that
# MOJO_HIP_GEMM_WAVES shows in the dense query at all (with N = 192 for four waves, N = 512 for seven)
K = (64, 128, 256, 384, 1024, 4096, 7168, 8192, 18432, 65536)
# N: below a tile, the weight stream's 64, not a multiple of 64 / of 256, one tile to a chip's worth
N = (16, 64, 132, 192, 512, 520, 1024, 4096, 7168, 14336)
GROUPS = (1, 4, 8, 64)


def dense_cases():
    """(m = 0 is left out of the recorded dense walk: the library this file was recorded from divides by the zero tiles of an
    empty product in its dense query where K has two K-tiles and N % 4 == 0, so it has no answer to record;
    tests/test_quant_plan_golden.py pins m = 0 to the 64 bytes that library answers for the other K)"""
    return itertools.product(M[1:], K, N)


def group_cases():
    return itertools.product(M, K, N, GROUPS)


# query name -> (C symbol, cases)
QUERIES = {
    "quant_gemm": ("mojo_hip_quant_gemm_workspace_bytes", dense_cases),
    "group_quant_gemm": ("mojo_hip_group_quant_gemm_workspace_bytes", group_cases),
}


def walk(query):
    """The argument tuples of ``query`` in grid order."""
    return QUERIES[query][1]()


def answers(lib, query):
    """array('q') of what ``query`` answers over its grid, under the environment in effect."""
    fn = getattr(lib, QUERIES[query][0])
    return array.array("q", (fn(*args) for args in walk(query)))


def digest(values):
    return hashlib.sha256(values.tobytes()).hexdigest()


class plan_env:
    """Walk the grid under one of ENVS: every switch the planners read is set or unset, both layers re-read them."""

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
