"""The scratch of sr3_vlb_terms_f32 / sr3_prior_bpd_f32 under the host checks every per-op scratch is held to
(tests/test_scratch_contract_cpu.py::test_per_op_scratch_is_checked_on_the_host, run here on this feature's rows): a scratch one byte
short is SR3_E_NOMEM with both sizes named, a misaligned one SR3_E_ALIGN; made-up pointers, nothing is launched."""
import pytest

import test_scratch_contract_cpu as SC
from vlb_scratch_rows import ROWS


@pytest.mark.parametrize('row', ROWS, ids=[r.id for r in ROWS])
def test_vlb_scratch_is_checked_on_the_host(row):
    SC.test_per_op_scratch_is_checked_on_the_host(row)
    from sr3_hip import lib as L
    assert row.entry in L.SIGNATURES and row.query in L.SIGNATURES
