"""`swa_packed.hip` (the linear instances of the prefill kernel) under the check of tests/test_isa_async_reads.py: no compiled
kernel touches a register that an LDS read issued from inline asm is still going to write.  The linear instances issue the K
and V^T fragment reads of `paged_prefill_body.h` from inline asm like the paged ones; their register allocation is their own."""
import os

import pytest

from test_isa_async_reads import _compile, _hipcc


@pytest.mark.skipif(_hipcc() is None, reason="no hipcc")
def test_no_register_of_an_in_flight_asm_lds_read_is_touched_in_the_linear_instances(tmp_path):
    import check_async_lds_reads as chk

    src, out, rc, err = _compile(("swa_packed.hip", str(tmp_path / "swa_packed.hip.s")))
    assert rc == 0, (src, err)
    reads, report = chk.check_file(out)
    assert not report, (src, report[:5])
    assert reads > 1000                                     # 96 instances: the pattern is really there
    assert os.path.getsize(out) > 1 << 20
