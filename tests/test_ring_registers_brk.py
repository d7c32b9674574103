"""The break-paf build of the streaming clip kernel is a translation unit of its own (k_liftover_brk.hip) with its load ring at v80..v95 and
no spill room: tools/check_ring.py on its assembly, as tests/test_ring_registers.py does for the other builds."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_ring  # noqa: E402

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not present")
def test_compiler_stays_out_of_the_break_builds_ring():
    text = check_ring.compile_to_asm(HIPCC, source="k_liftover_brk.hip")
    bad = check_ring.check_assembly(text, 1, check_ring.RING)
    assert not bad, bad[:5]
    assert check_ring.spills(text)["_Z24rb_k_liftover_stream_brk14rb_lift_params"][1] == 0  # no vector register spilled to scratch
