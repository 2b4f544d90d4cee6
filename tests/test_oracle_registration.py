"""`import oracle`, and nothing else, registers a ``torch`` backend for every op of the package.

Run in a fresh interpreter, so that no test module collected earlier can have registered anything: every `Mojo*` name of
`mojo_opset_amd.__all__` and every name of `BEYOND_SURVEY_OPS` must answer ``get_backend_impl("torch", strict=True)`` with a
class named ``Torch<Name>``."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = """
import sys
import oracle
assert "mojo_opset_amd" in sys.modules            # imported by the oracle, not by this script
mo = sys.modules["mojo_opset_amd"]
names = [n for n in mo.__all__ if n.startswith("Mojo") and n not in ("MojoOperator", "MojoBackendRegistry")]
names += list(mo.BEYOND_SURVEY_OPS)
assert len(names) == len(set(names)) and len(mo.BEYOND_SURVEY_OPS) == 16, names
for name in names:
    got = getattr(mo, name).get_backend_impl("torch", strict=True).__name__
    assert got == "Torch" + name[4:], (name, got)
print("registered", len(names))
"""


def test_import_oracle_alone_registers_every_torch_backend():
    run = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, capture_output=True, text=True, timeout=120)   # -c: cwd is on sys.path
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.split()[-2] == "registered" and int(run.stdout.split()[-1]) > 16, run.stdout
